"""What the five entries that take a caller's table -- bp_stark_prove_trace, bp_air_port_products, bp_air_check_trace,
bp_stark_prove_table_set, bp_check_table_set -- refuse about it, on the arguments alone: a null trace, a column stride
shorter than the trace, constant columns missing where the AIR reads some, public inputs missing where it reads them, a
public input that is no canonical field word.  Each is BP_ERR_INVALID_INPUT (-2) under the entry's own name, and comes
before any device call: nothing here needs a GPU, and the pointers that stand for device memory are never read."""
import ctypes as C

import numpy as np
import pytest

import air_program_cases as cases
from air_program_cases import P
from proof_protocol_decoder_amd._lib import SetReport
from proof_protocol_decoder_amd.air_program import ALL_ROWS, FIRST_ROW, Builder

ENTRIES = ["bp_stark_prove_trace", "bp_air_port_products", "bp_air_check_trace", "bp_stark_prove_table_set", "bp_check_table_set"]
LOG_N = 5
N = 1 << LOG_N
GOOD_PUB = (1, 2, 3, 4)
# refusal -> the one argument that is wrong (the others are fine), and a word the message has to say
REFUSALS = {
    "null trace": (dict(trace=False), "null"),
    "short stride": (dict(stride=N - 1), "stride"),
    "no constants": (dict(consts=False), "constant columns|null argument"),
    "no public inputs": (dict(pub=None), "public inputs"),
    "non-canonical public input": (dict(pub=(1, P, 3, 4)), "non-canonical"),
}


@pytest.fixture(scope="module")
def bpg():
    """the package with its library loaded: nothing here touches a device"""
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    return pkg


@pytest.fixture(scope="module")
def table(bpg):
    """a program that reads a constant column and a public input and has a looking and a looked port (a set of this one
    table links them to each other)"""
    b = Builder(8, n_const=1, n_public=1)
    bit = b.family(1, ALL_ROWS, 2)
    first = b.family(1, FIRST_ROW, 1)
    b.unit()
    b.emit(bit, b.loc(0) * b.loc(0) - b.loc(0))
    b.emit(first, b.loc(1) - b.pub(0) - b.cst(0))
    b.port(b.loc(0), [b.loc(1)])
    b.port(b.loc(0), [b.loc(2)])
    reg = bpg.ops.air_register(b.assemble())
    return reg, cases.cfg_for(reg, LOG_N, num_queries=6, pow_bits=6)


def call(bpg, entry, reg, cfg, trace=True, stride=N, consts=True, pub=GOOD_PUB):
    """(status, message) of `entry` on the table; trace / consts: whether the pointer is given"""
    L = bpg.lib()
    stand_in = np.zeros(8, dtype=np.uint64)         # stands for device memory: every call here ends before it is looked at
    ptr = stand_in.ctypes.data
    d_trace, d_consts = ptr if trace else None, ptr if consts else None
    pub_arr = (C.c_uint64 * 4)(*pub) if pub is not None else None
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    if entry == "bp_stark_prove_trace":
        rc = L.bp_stark_prove_trace(reg, C.byref(cfg), d_trace, stride, d_consts, pub_arr, 0, C.byref(out), C.byref(n))
    elif entry == "bp_air_port_products":
        rc = L.bp_air_port_products(reg, C.byref(cfg), d_trace, stride, d_consts, pub_arr, (C.c_uint64 * 4)(5, 6, 7, 8), ptr, None)
    elif entry == "bp_air_check_trace":
        n_rows, n_viol = C.c_uint64(), C.c_uint32()
        rc = L.bp_air_check_trace(reg, C.byref(cfg), d_trace, stride, d_consts, pub_arr, 0, C.byref(n_rows), None, None, 0, C.byref(n_viol), None)
    else:
        ta, la, keep = bpg.ops._set_arguments([{"air_id": reg, "cfg": cfg, "pub": pub}], [([(0, 0)], (0, 1))])
        ta[0].d_trace, ta[0].stride, ta[0].d_consts = d_trace, stride, d_consts
        if entry == "bp_stark_prove_table_set":
            rc = L.bp_stark_prove_table_set(ta, 1, la, 1, 0, 0, C.byref(out), C.byref(n))
        else:
            rc = L.bp_check_table_set(ta, 1, la, 1, 0, C.byref(SetReport()))
    assert not out and n.value == 0                 # no buffer with a refusal
    return rc, L.bp_last_error().decode()


@pytest.mark.parametrize("refusal", list(REFUSALS))
@pytest.mark.parametrize("entry", ENTRIES)
def test_a_caller_table_is_refused_on_its_arguments_alone(bpg, table, entry, refusal):
    import re
    wrong, says = REFUSALS[refusal]
    rc, message = call(bpg, entry, *table, **wrong)
    assert rc == -2, (rc, message)
    assert message.startswith(entry + ": ") and re.search(says, message), message
    if entry.endswith("table_set"):
        assert "table 0: " in message, message
