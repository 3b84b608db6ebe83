"""The exponentiation table on the GPU: the witness kernel (csrc/arithmetic_exp.hip) against the independent model of
tests/arithmetic_exp_model.py word for word, then the shipped program -- the first whose families span rows -- through
the run-time stack: the device checker, the prover and the verifier, the port's running products, and table sets in which
a caller's table looks exponentiations up.  Everything is exact.  2^5 rows, except where an operation needs more: the
edge lists with their 256-row operations take 2^9, the claim about an exponent of 65 bits 2^7.  What holds for every
shipped table -- the proof of the 2^5-row trace, the port's running products -- is word_tables.proof_tests over this
table's record, and the looking table and the accept and refuse helpers are imported from there; the rest is its own,
because the operations span rows.  CPU side: tests/test_arithmetic_exp.py."""
import numpy as np
import pytest

import air_program_cases as cases
import arithmetic_exp_model as model
from air_program_port_cases import LINK, cfg_of
from proof_protocol_decoder_amd import arithmetic_exp as ex
from util import to_dev, to_host
from word_tables import (EXPONENTIATION, assert_equal_word_for_word, dev_starts, proof_tests, proves_and_verifies,
                         refused_by_the_pre_flight_the_prover_and_the_verifier, renamed, table_set, with_traces)

globals().update(renamed(proof_tests(EXPONENTIATION), test_the_edge_trace_proves_and_verifies="test_the_small_trace_proves_and_verifies"))

N_COLS, device_trace = EXPONENTIATION.n_cols, EXPONENTIATION.device_trace
# one wrong witness per family group: the chain's two ends, its four transitions, the two products, the choice of out, the
# flags, the range checks
REJECTED = ("chain_cut_short", "chain_off_the_traces_end", "r_not_one_on_a_first_row", "next_p_not_the_square",
            "multiply_skipped_on_a_one_bit", "result_not_handed_on", "exponent_bit_dropped_in_the_shift", "res_changed_in_mid_chain",
            "res_not_out_on_the_last_row", "m_not_the_product", "s_not_the_square", "carry_out_of_range", "limb_of_two_to_the_16",
            "non_bit_in_e", "non_bit_in_m", "g_on_a_row_that_is_not_first", "flag_that_is_no_bit")
GROUPS = [e for e in model.CATALOGUE if e[0] in REJECTED]
assert len(GROUPS) == len(REJECTED) and {f for e in GROUPS for _, f in e[2]} == {name for name, _ in model.FAMILIES}

LISTS = {"edges-2^9": (model.edge_ops, 9), "a-multiply-on-every-row-2^9": (model.edge_ops_tail, 9), "small-2^5": (model.small_ops, 5),
         "to-the-last-row-2^5": (model.small_ops_to_the_end, 5), "random-2^5": (lambda: model.random_ops(32, 0xE8B1), 5)}


@pytest.mark.parametrize("which", LISTS)
def test_the_device_witness_is_the_model_and_the_checker_is_clean(bpg, reg, which):
    make, log_n = LISTS[which]
    ops = make()
    t = device_trace(bpg, ops, log_n)
    assert_equal_word_for_word(to_host(t), model.trace_of(ops, log_n))
    got = bpg.ops.check_air_trace(reg, t)
    assert got.ok and got.n_violations == 0, got


def test_the_kernel_writes_every_cell_and_ignores_what_it_should(bpg):
    """a trace buffer full of ones before the call; bits 9 .. 63 of word 0 and a padding operation's words change nothing"""
    import torch
    ops = model.small_ops()
    words, starts = ex.pack_ops(ops, 5)
    want = model.trace_of(ops, 5)
    words[:, 0] |= np.uint64(0xABCDEF << 9)
    padding = [i for i, op in enumerate(ops) if op[0] != model.EXP]
    assert any(int(words[i, 1:].any()) and ops[i][3] for i in padding)           # a padding operation carries junk
    out = torch.full((N_COLS, 32), -1, dtype=torch.int64, device="cuda")
    d_words, d_starts = to_dev(words), dev_starts(starts)
    assert bpg.lib().bp_arithmetic_exp_trace(d_words.data_ptr(), len(ops), d_starts.data_ptr(), 5, out.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream) == 0
    got = to_host(out)
    assert_equal_word_for_word(got, want)
    for i in (10, 11, 28, 29, 30, 31):   # all zero except last = 1
        assert [c for c in range(N_COLS) if got[c, i]] == [model.LAST]


def test_wrong_prefix_sums_give_a_trace_the_checker_refuses(bpg, reg):
    """the padding operation of the 2^5-row list starts a row early, so (2, 0b101101) has five rows for its six: the lane of
    row 8 takes `last` from its exponent, 0b10, not from the sums, and the row after it is not its step.  The run ends as
    any other"""
    import torch
    ops = model.small_ops()
    words, starts = ex.pack_ops(ops, 5)
    assert int(starts[3]) == 10 and ops[2][2] == 0b101101
    starts[3] -= 1
    t = bpg.ops.arithmetic_exp_trace(5, to_dev(words), dev_starts(starts))
    torch.cuda.synchronize()
    got = bpg.ops.check_air_trace(reg, t, max_viol=512)
    assert not got.ok and got.rows == [8]
    assert {ex.FAMILIES[v.family][0] for v in got.violations} == {"step_p", "step_r", "step_e", "step_res"}
    host = to_host(t)
    want = model.trace_of(ops, 5)
    assert [i for i in range(32) if (host[:, i] != want[:, i]).any()] == [9] and not host[model.LAST, 8]


@pytest.mark.parametrize("entry", GROUPS, ids=[e[0] for e in GROUPS])
def test_the_proof_of_a_wrong_witness_is_rejected(bpg, reg, at_2_5, entry):
    """the rows a forgery rewrites -- one, or two that follow each other, or a chain's -- replace those of the device's
    trace: the device checker names the rows and the families, the prover proves what it is given, the verifier rejects at
    zeta"""
    ops, t = at_2_5
    honest, forged = model.trace_of(ops, 5), model.forged(entry)
    rows = [i for i in range(32) if (honest[:, i] != forged[:, i]).any()]
    assert rows
    bad = t.clone()
    for i in rows:
        bad[:, i] = to_dev(forged[:, i])
    got = bpg.ops.check_air_trace(reg, bad, max_viol=512)
    assert {(v.row, ex.FAMILIES[v.family][0]) for v in got.violations} == entry[2]
    assert got.rows == sorted({row for row, _ in entry[2]})
    cfg = cfg_of(reg, 5)
    assert cases.verify(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, bad)) == -5
    assert b"constraint check at zeta" in bpg.lib().bp_last_error()


# ---------------------------------------------------------------------------------------------- table sets
# one looking table claims one operation, the only one of its table: (base, exponent, the classic wrong result, log_n)
STORIES = {"the_exponent_masked_to_a_byte": (2, 256, 1, 4),                      # 2^(256 mod 256)
           "the_exponent_masked_to_64_bits": (3, (1 << 64) + 1, 3, 7),           # 3^((2^64 + 1) mod 2^64)
           "zero_to_the_zero": (0, 0, 0, 4)}


def test_a_callers_table_looks_the_operations_up(bpg, reg):
    """the 2^5-row list exposes five operations; the caller claims them in another order"""
    ops = model.small_ops()
    asked = [(o[1], o[2], pow(o[1], o[2], 1 << 256)) for o in ops if o[0] == model.EXP and o[3]]
    assert len(asked) == 5
    tables, traces, _ = table_set(bpg, EXPONENTIATION, reg, ops, asked[::-1], 0xE875)
    got = bpg.ops.check_table_set(with_traces(tables, traces), LINK)
    assert got.ok and got.links[0].holds and (got.links[0].n_looking, got.links[0].n_looked) == (5, 5), got
    proves_and_verifies(bpg, tables, traces)


@pytest.mark.parametrize("story", STORIES)
def test_an_honest_claim_is_accepted(bpg, reg, story):
    base, e, _, log_n = STORIES[story]
    tables, traces, _ = table_set(bpg, EXPONENTIATION, reg, [(model.EXP, base, e, 1)], [(base, e, pow(base, e, 1 << 256))], 0xE876, log_n)
    proves_and_verifies(bpg, tables, traces)


@pytest.mark.parametrize("story", STORIES)
def test_a_wrong_claim_is_refused(bpg, reg, story):
    """EXP(2, 256) = 1, EXP(3, 2^64 + 1) = 3, EXP(0, 0) = 0: the whole exponent decides, and 0^0 = 1"""
    base, e, wrong, log_n = STORIES[story]
    assert wrong != pow(base, e, 1 << 256)
    tables, traces, rows = table_set(bpg, EXPONENTIATION, reg, [(model.EXP, base, e, 1)], [(base, e, wrong)], 0xE877, log_n)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, rows[0], 0)


def test_an_operation_that_is_not_exposed_cannot_be_looked_up(bpg, reg):
    tables, traces, rows = table_set(bpg, EXPONENTIATION, reg, [(model.EXP, 3, 5, 0)], [(3, 5, 243)], 0xE878, 4)
    refused_by_the_pre_flight_the_prover_and_the_verifier(bpg, tables, traces, rows[0], -1)


# ---------------------------------------------------------------------------------------------- refusals
def test_no_operations_give_an_all_padding_trace_that_verifies(bpg, reg):
    words, starts = ex.pack_ops([], 5)
    t = bpg.ops.arithmetic_exp_trace(5, to_dev(words), dev_starts(starts))
    host = to_host(t)
    assert host.shape == (N_COLS, 32) and (host[model.LAST] == 1).all() and int(host.sum()) == 32
    assert bpg.ops.check_air_trace(reg, t).ok
    cfg = cases.cfg_for(reg, 5)
    bpg.ops.stark_verify_air(reg, cfg, bpg.ops.stark_prove_trace(reg, cfg, t))


def test_refusals(bpg):
    import torch
    from proof_protocol_decoder_amd._lib import BpgError
    trace = bpg.ops.arithmetic_exp_trace
    words, starts = ex.pack_ops(model.small_ops(), 5)
    good, good_starts = to_dev(words), dev_starts(starts)
    with pytest.raises(ValueError, match=r"\[n_ops, 9\]"):
        trace(5, torch.zeros((8, 8), dtype=torch.int64, device="cuda"), good_starts)
    with pytest.raises(ValueError, match=r"starts is \[9\]"):
        trace(5, good, good_starts[:8])
    with pytest.raises(ValueError, match="int32"):
        trace(5, good, good_starts.to(torch.int64))
    with pytest.raises(ValueError, match="int64"):
        trace(5, good.to(torch.int32), good_starts)
    with pytest.raises(ValueError, match="device tensors"):
        trace(5, good.cpu(), good_starts)
    with pytest.raises(ValueError, match="int32"):
        trace(5, good, good_starts.cpu())
    many = torch.zeros((17, 9), dtype=torch.int64, device="cuda")
    with pytest.raises(BpgError) as e:
        trace(4, many, torch.zeros(18, dtype=torch.int32, device="cuda"))
    assert e.value.code == -2 and "17 operations in 2^4 rows" in e.value.message
    # refused before anything is launched, so the pointers are never read
    entry = bpg.lib().bp_arithmetic_exp_trace
    out = torch.zeros(8, dtype=torch.int64, device="cuda")
    for log_n in (3, 27):
        assert entry(good.data_ptr(), 8, good_starts.data_ptr(), log_n, out.data_ptr(), None) == -2
        assert b"log_n out of range" in bpg.lib().bp_last_error()
    assert entry(good.data_ptr(), 8, good_starts.data_ptr(), 5, None, None) == -2 and b"null output" in bpg.lib().bp_last_error()
    assert entry(None, 8, good_starts.data_ptr(), 5, out.data_ptr(), None) == -2 and b"null operations" in bpg.lib().bp_last_error()
    assert entry(good.data_ptr(), 8, None, 5, out.data_ptr(), None) == -2 and b"null starts" in bpg.lib().bp_last_error()
    assert entry(good.data_ptr(), 33, good_starts.data_ptr(), 5, out.data_ptr(), None) == -2
    torch.cuda.synchronize()
    assert int(out.sum()) == 0
