"""The signed table on the GPU: the witness kernel (csrc/arithmetic_sdiv.hip) against the independent row model of
tests/arithmetic_sdiv_model.py word for word, then the shipped program through the run-time stack -- the device checker,
the prover and the verifier, the port's running products, and table sets in which a caller's table looks signed
divisions up.  Everything is exact, at 2^5 rows throughout.  The bodies restate word_tables.gpu_tests for this table's
record; what holds unchanged -- the looking table, one_claim, the accept and refuse helpers -- is imported from there.
CPU side: tests/test_arithmetic_sdiv.py."""
from types import SimpleNamespace

import numpy as np
import pytest

import air_program_cases as cases
import arithmetic_sdiv_model as model
from air_program_port_cases import cfg_of
from proof_protocol_decoder_amd import arithmetic_sdiv as sd
from util import to_dev, to_host
from word_tables import (assert_equal_word_for_word, device_trace, one_claim, proves_and_verifies,
                         refused_by_the_pre_flight_the_prover_and_the_verifier)

pytestmark = pytest.mark.gpu

# what word_tables' generic helpers read of a table's record: the port has the division table's shape (50 elements, a
# looking table of 56 columns)
SIGNED = SimpleNamespace(name="signed", module=sd, model=model, trace_op="arithmetic_sdiv_trace", width=50, looker_cols=56)
N_COLS = 2499
n_ = model.to_word
# one wrong witness per family group: the core, the three negations, the sign, the zero test, the flags, the range checks
REJECTED = ("floor_for_truncation", "remainder_with_the_divisors_sign", "result_with_the_sign_dropped",
            "negated_result_with_the_last_carry_cleared", "magnitude_not_taken", "magnitude_limb_out_of_range",
            "remainder_equal_to_the_divisor", "wrap_in_the_high_columns", "no_zero_flag_on_y_zero", "neg_flipped", "both_flags",
            "exposed_padding_row", "limb_of_two_to_the_16", "remainder_as_quotient", "non_bit_in_res", "non_bit_in_a_carry")
GROUPS = [e for e in model.CATALOGUE if e[0] in REJECTED]
assert len(GROUPS) == len(REJECTED)


@pytest.fixture(scope="module")
def reg(bpg):
    return sd.register()


@pytest.fixture(scope="module")
def edge(bpg):
    """(operations, device trace) of the 2^5-row edge list"""
    ops = model.edge_ops()
    return ops, device_trace(bpg, SIGNED, ops)


@pytest.mark.parametrize("which", ["edges", "random"])
def test_the_device_witness_is_the_model_and_the_checker_is_clean(bpg, reg, which):
    ops = {"edges": model.edge_ops, "random": lambda: model.random_ops(32, 0x5D1F)}[which]()
    assert len(ops) == 32
    t = device_trace(bpg, SIGNED, ops)
    assert_equal_word_for_word(to_host(t), model.trace_of(ops))
    got = bpg.ops.check_air_trace(reg, t)
    assert got.ok and got.n_violations == 0, got


def test_the_kernel_writes_every_cell_and_ignores_what_it_should(bpg):
    """a trace buffer full of ones before the call; bits 9 .. 63 of word 0 and a padding row's operands change nothing"""
    import torch
    ops = model.edge_ops()
    words = sd.pack_inputs(ops)
    want = model.trace_of(ops)
    words[:, 0] |= np.uint64(0xABCDEF << 9)
    padding = [i for i, op in enumerate(ops) if op[0] not in model.LIVE]
    assert any(int(words[i, 1:].any()) for i in padding) and any(ops[i][3] for i in padding)   # padding rows carry junk
    out = torch.full((N_COLS, 32), -1, dtype=torch.int64, device="cuda")
    d_words = to_dev(words)
    assert bpg.lib().bp_arithmetic_sdiv_trace(d_words.data_ptr(), 5, out.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    got = to_host(out)
    assert_equal_word_for_word(got, want)
    for i in padding:   # all zero except z = 1
        assert [c for c in range(N_COLS) if got[c, i]] == [model.Z]


def test_the_edge_trace_proves_and_verifies(bpg, reg, edge):
    _, t = edge
    cfg = cases.cfg_for(reg, 5)
    assert (cfg.n_cols, cfg.rate_bits, cfg.deg_pow) == (N_COLS, 1, 1)
    proof = bpg.ops.stark_prove_trace(reg, cfg, t)
    assert int(proof[4]) == 2 and int(proof[14]) == reg                         # two auxiliary columns: the port's products
    bpg.ops.stark_verify_air(reg, cfg, proof)
    assert cases.verify(7, cases.cfg_for(7, 5), proof) == -5                    # ... under its own id only


@pytest.mark.parametrize("entry", GROUPS, ids=[e[0] for e in GROUPS])
def test_the_proof_of_a_wrong_witness_is_rejected(bpg, reg, edge, entry):
    """the forged row replaces row 9 of the device's edge trace: the device checker names it, the prover proves what it is
    given, the verifier rejects at zeta"""
    _, t = edge
    bad = t.clone()
    bad[:, 9] = to_dev(np.array(model.forged(entry), dtype=np.uint64))
    got = bpg.ops.check_air_trace(reg, bad, max_viol=512)
    assert got.rows == [9] and {sd.FAMILIES[v.family][0] for v in got.violations} == entry[3]
    cfg = cfg_of(reg, 5)
    assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, bad)) == -5
    assert b"constraint check at zeta" in bpg.lib().bp_last_error()


def test_the_ports_running_products_are_the_builders(bpg, reg, edge):
    ops, t = edge
    assert 0 < sum(1 for op in ops if op[0] in model.LIVE and op[3]) < 32
    rng = np.random.default_rng(0x5D7C)
    ctl = [int(v) for v in rng.integers(2, model.P, size=4, dtype=np.uint64)]
    got = to_host(bpg.ops.air_port_products(reg, t, ctl))
    want = sd.program().port_running_columns(model.trace_of(ops), ctl)
    assert got.shape == (2, 32) and [[int(v) for v in col] for col in got] == want
    assert int(got[0, 0]) not in (0, 1) and int(got[0, 0]) != int(got[1, 0])


# ---------------------------------------------------------------------------------------------- table sets
# one looking table claims one row, row 9 of the edge list (a padding row, nothing else exposed): (operation, the honest
# result, the classic wrong one)
STORIES = {"sdiv_truncates": ((model.SDIV, n_(-7), 2), n_(-3), n_(-4)),
           "smod_has_the_sign_of_x": ((model.SMOD, n_(-7), 2), n_(-1), 1),
           "sdiv_of_the_most_negative_word_by_minus_one": ((model.SDIV, 1 << 255, n_(-1)), 1 << 255, 0),
           "sdiv_by_zero": ((model.SDIV, 5, 0), 0, None)}
for _operation, _honest, _ in STORIES.values():
    assert model.statement(*_operation) == _honest


@pytest.mark.parametrize("story", STORIES)
def test_an_honest_claim_is_accepted(bpg, reg, story):
    operation, honest, _ = STORIES[story]
    tables, traces, _ = one_claim(bpg, SIGNED, reg, 9, operation, 1, honest, 0x5D76)
    proves_and_verifies(bpg, tables, traces)


@pytest.mark.parametrize("story", [s for s in STORIES if STORIES[s][2] is not None])
def test_a_wrong_claim_is_refused(bpg, reg, story):
    """the floor for the truncation, the remainder with the divisor's sign, 0 for the quotient 2^255"""
    operation, _, wrong = STORIES[story]
    tables, traces, row = one_claim(bpg, SIGNED, reg, 9, operation, 1, wrong, 0x5D77)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, 9)


def test_an_operation_that_is_not_exposed_cannot_be_looked_up(bpg, reg):
    operation, honest, _ = STORIES["sdiv_truncates"]
    tables, traces, row = one_claim(bpg, SIGNED, reg, 9, operation, 0, honest, 0x5D78)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, row, -1)


def test_refusals(bpg):
    import torch
    from proof_protocol_decoder_amd._lib import BpgError
    trace = bpg.ops.arithmetic_sdiv_trace
    good = to_dev(sd.pack_inputs(model.edge_ops()))
    with pytest.raises(BpgError) as e:
        trace(5, None)
    assert e.value.code == -2 and "null inputs" in e.value.message
    with pytest.raises(ValueError, match=r"\[32, 9\]"):
        trace(5, good[:31])
    with pytest.raises(ValueError, match=r"\[16, 9\]"):
        trace(4, good)
    with pytest.raises(ValueError, match=r"\[32, 9\]"):
        trace(5, torch.zeros((32, 8), dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError, match="int64"):
        trace(5, good.to(torch.int32))
    with pytest.raises(ValueError, match="device tensors"):
        trace(5, good.cpu())
    # heights outside 4 .. 26 are refused before anything is launched, so the pointers are never read
    entry = bpg.lib().bp_arithmetic_sdiv_trace
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    for log_n in (3, 27):
        assert entry(good.data_ptr(), log_n, out.data_ptr(), None) == -2
        assert b"log_n out of range" in bpg.lib().bp_last_error()
    assert entry(good.data_ptr(), 5, None, None) == -2
    assert entry(None, 5, out.data_ptr(), None) == -2 and b"null inputs" in bpg.lib().bp_last_error()
    torch.cuda.synchronize()
    assert int(out.sum()) == 0
