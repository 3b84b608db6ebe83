"""Lookup ports of run-time AIRs and table sets, the part that needs no GPU (csrc/air_program.cpp: the "BPGAIRP2"
validator; bp_air_describe; the argument checks of bp_stark_prove_table_set / bp_stark_verify_table_set, which refuse a
bad statement before a device is touched).  GPU side: tests/test_gpu_air_program_ports.py."""
import re

import numpy as np
import pytest

import air_program_cases as cases
import air_program_port_cases as pc
from proof_protocol_decoder_amd import air_program as ap
from proof_protocol_decoder_amd._lib import BpgError


@pytest.fixture(scope="module")
def bpg():
    """the package with its library loaded: nothing here touches a device"""
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    return pkg


def layout(w):
    """word offsets of a "BPGAIRP2" program: family table, port table, unit offsets, code; and its counts"""
    assert int(w[0]) == ap.MAGIC2
    n_fam, n_units, n_ports = int(w[6]), int(w[8]), int(w[10])
    fam0 = 11
    port0 = fam0 + 4 * n_fam
    off0 = port0 + n_ports
    code0 = off0 + n_units + n_ports + 1
    return dict(fam0=fam0, port0=port0, off0=off0, code0=code0, n_units=n_units, n_ports=n_ports)


def unit_words(w, u):
    """[(word offset, op, dst, a, b)] of unit u (port unit l = n_units + l), immediates' constant words skipped"""
    L = layout(w)
    pc_, end = L["code0"] + int(w[L["off0"] + u]), L["code0"] + int(w[L["off0"] + u + 1])
    out = []
    while pc_ < end:
        c = int(w[pc_])
        out.append((pc_, c & 0xff, (c >> 8) & 0xff, (c >> 16) & 0xffffff, c >> 40))
        pc_ += 2 if c & 0xff == ap.OP_IMM else 1
    return out


def word(op, d=0, a=0, b=0):
    return np.uint64(op | d << 8 | a << 16 | b << 40)


def refused(bpg, w, off, what):
    with pytest.raises(BpgError) as e:
        bpg.ops.air_register(w)
    assert e.value.code == -2 and re.search(r"word %d: " % off, e.value.message) and re.search(what, e.value.message), \
        (off, e.value.message)


def test_a_builder_without_ports_emits_the_bytes_and_ids_it_emitted_before(bpg):
    """the ids are those of the commit before ports existed (AIR 4's transcription is also named in
    profiles/air_program_k5.txt)"""
    for make, want in ((cases.arithmetic_program, 0xFCCC1196), (cases.memory_program, 0xB98F47A5), (cases.fibonacci_program, 0xCDADB07B)):
        w = make().assemble()
        assert int(w[0]) == ap.MAGIC == int.from_bytes(b"BPGAIRP1", "little")
        assert bpg.ops.air_register(w) == want
    b = cases.memory_program()
    n1 = b.assemble().size
    b.port(b.loc(44), [b.loc(0)])
    w2 = b.assemble()
    assert int(w2[0]) == ap.MAGIC2 and w2.size > n1 and bpg.ops.air_register(w2) != 0xB98F47A5


def test_p2_header_round_trips_through_register_and_describe(bpg):
    b = pc.flag_program(width=3, ports=2)
    w = b.assemble()
    L = layout(w)
    assert (L["n_units"], L["n_ports"]) == (1, 2) and [int(v) for v in w[L["port0"]:L["off0"]]] == [3, 3]
    assert w.size == L["code0"] + int(w[9]) and int(w[L["off0"] + 3]) == int(w[9])
    reg = bpg.ops.air_register(w)
    assert reg & 0x80000000 and bpg.ops.air_register(w) == reg
    d = bpg.ops.air_describe(reg)
    assert (d.n_cols, d.n_aux, d.n_air_constraints, d.n_ctl_constraints, d.n_units) == (8, 4, b.n_constraints, 10, 1)
    fams = [(f.first_index, f.count, f.kind, f.degree) for f in d.families[:d.n_families]]
    assert fams[:len(b.families)] == b.families
    base = b.n_constraints
    # per port: the filter bit on all rows, then per challenge set transition z - z' term, last row z - term
    assert fams[len(b.families):] == [(base + 5 * l + k, 1, kind, deg) for l in range(2)
                                      for k, (kind, deg) in enumerate([(0, 2), (1, 3), (3, 2), (1, 3), (3, 2)])]
    # the memory table's transcription reports the built-in's own lookup families
    m = bpg.ops.air_describe(bpg.ops.air_register(pc.memory_port_program().assemble()))
    d3 = bpg.ops.air_describe(3)
    fam = lambda d: [(f.first_index, f.count, f.kind, f.degree) for f in d.families[:d.n_families]]
    assert fam(m) == fam(d3) and (m.n_aux, m.n_ctl_constraints) == (d3.n_aux, d3.n_ctl_constraints) == (2, 5)
    # a "BPGAIRP2" program without ports keeps the one constant product
    w0 = np.concatenate([[np.uint64(ap.MAGIC2)], cases.fibonacci_program().assemble()[1:10], [np.uint64(0)],
                         cases.fibonacci_program().assemble()[10:]]).astype(np.uint64)
    d0 = bpg.ops.air_describe(bpg.ops.air_register(w0))
    assert (d0.n_aux, d0.n_ctl_constraints) == (1, 2)


def test_builder_evaluates_ports_over_python_integers():
    b = pc.flag_program(width=2, ports=2)
    row, nxt = [1, 10, 20, 7, 0, 0, 0, 0], [0] * 8
    assert b.evaluate_ports(row, nxt) == [(1, [10, 20]), (1, [11, 21])]
    with pytest.raises(ValueError, match="do not fit"):
        q = pc.flag_program(ports=0, degree=3)
        q.port(q.loc(0) * q.loc(0), [q.loc(1)])
        q.assemble()


def test_validator_refuses_bad_ports_with_the_word_offset(bpg):
    base = pc.flag_program(width=3, ports=2).assemble()
    L = layout(base)
    u0 = unit_words(base, 0)
    p0 = unit_words(base, L["n_units"])            # port 0's unit: no immediates
    ports = [x for x in p0 if x[1] == ap.OP_PORT]
    assert [x[2] for x in ports] == [0, 1, 2, 3] and all(x[3] == 0 for x in ports)
    bpg.ops.air_register(base)

    def mutated(at, value):
        w = base.copy()
        w[at] = value
        return w

    at, op, d, a, b = ports[3]
    # a tuple slot never written (slot 3's word writes slot 2 again)
    refused(bpg, mutated(at, word(ap.OP_PORT, 2, 0, b)), L["off0"] + L["n_units"], "slot 3 .* never written")
    # a slot beyond the tuple
    refused(bpg, mutated(at, word(ap.OP_PORT, 4, 0, b)), at, "slot 4 of port 0")
    # emit in a port unit; port in a constraint unit; a port unit that names another port
    refused(bpg, mutated(at, word(ap.OP_EMIT, 0, 0, b)), at, "emit in port unit 0")
    e_at, _, e_d, e_a, e_b = next(x for x in u0 if x[1] == ap.OP_EMIT)
    refused(bpg, mutated(e_at, word(ap.OP_PORT, 0, 0, e_b)), e_at, "port in constraint unit 0")
    refused(bpg, mutated(at, word(ap.OP_PORT, 3, 1, b)), at, "unit of port 0 feeds port 1")
    # 9 ports; n_tuple 0 and 129
    refused(bpg, mutated(10, np.uint64(9)), 10, "n_ports = 9")
    refused(bpg, mutated(L["port0"], np.uint64(0)), L["port0"], "n_tuple = 0")
    refused(bpg, mutated(L["port0"] + 1, np.uint64(129)), L["port0"] + 1, "n_tuple = 129")
    # a register read before it is written: port 0's unit starts with its port word instead of the load it reads
    w = base.copy()
    w[p0[0][0]], w[p0[1][0]] = base[p0[1][0]], base[p0[0][0]]
    assert p0[0][1] == ap.OP_LOC and p0[1][1] == ap.OP_PORT
    refused(bpg, w, p0[0][0], "read before unit 1 writes it")
    # an operation the format does not have
    refused(bpg, mutated(at, word(11, 0, 0, b)), at, "unknown operation 11")
    # "BPGAIRP1" has no port operation
    p1 = cases.fibonacci_program().assemble()
    first = 10 + 4 * int(p1[6]) + int(p1[8]) + 1
    p1[first] = word(ap.OP_PORT, 0, 0, 0)
    refused(bpg, p1, first, "unknown operation 10")


def test_validator_refuses_ports_whose_degrees_do_not_fit(bpg):
    """2 deg f <= degree, 1 + deg f + deg t <= degree, deg f + deg t <= the last-row bound: refused at the port unit's
    offset word"""
    def at_unit(w, l):
        L = layout(w)
        return L["off0"] + L["n_units"] + l

    # a filter of degree 2 in a degree-3 program
    b = pc.flag_program(ports=0, degree=3)
    b.port(b.loc(0) * b.loc(0), [b.loc(1)])
    w = b.assemble(check_ports=False)
    assert int(w[4]) == 3
    refused(bpg, w, at_unit(w, 0), "degree violation: port 0 has a filter of degree 2")
    # a quadratic tuple element in a degree-3 program
    b = pc.flag_program(ports=1, degree=3)
    b.port(b.loc(0), [b.loc(1), b.loc(2) * b.loc(3)])
    w = b.assemble(check_ports=False)
    refused(bpg, w, at_unit(w, 1), "degree violation: port 1 has a filter of degree 1 and a tuple of degree 2")
    # the same tuple fits a degree-9 program: 1 + 1 + 2 <= 9 and 1 + 2 <= 8
    b = pc.flag_program(ports=0, degree=9)
    b.port(b.loc(0), [b.loc(1), b.loc(2) * b.loc(3)])
    d = bpg.ops.air_describe(bpg.ops.air_register(b.assemble()))
    assert [(f.kind, f.degree) for f in d.families[d.n_families - 5:d.n_families]] == [(0, 2), (1, 4), (3, 3), (1, 4), (3, 3)]
    # ... and a tuple of degree 8 does not: z - z' term would have degree 10 (the last-row bound, deg f + deg t <= 8
    # there, is implied by this rule at every degree a program can declare: it never refuses on its own)
    b = pc.flag_program(ports=0, degree=9)
    t = b.loc(1)
    for _ in range(7):
        t = t * b.loc(2)
    b.port(b.loc(0), [t])
    w = b.assemble(check_ports=False)
    refused(bpg, w, at_unit(w, 0), "a tuple of degree 8, z - z' term must fit the program's degree 9")
    # a program with ports has at most 21 families of its own: the description holds both lists
    b = pc.flag_program(width=1, n_cols=8, ports=0)
    for _ in range(19):
        b.emit(b.family(1, 0, 1), b.loc(7))
    assert len(b.families) == 22
    assert bpg.ops.air_register(b.assemble()) & 0x80000000
    b.port(b.loc(0), [b.loc(1)])
    with pytest.raises(ValueError, match="at most 21"):
        b.assemble()
    refused(bpg, b.assemble(check_ports=False), 6, "at most 21 families")


def test_eight_ports_register_and_their_families_are_summarised(bpg):
    """5 families per port where they fit bp_air_desc.families[24] behind the program's own, else three interleaved ones"""
    b = pc.flag_program(ports=8)
    d = bpg.ops.air_describe(bpg.ops.air_register(b.assemble()))
    base = b.n_constraints
    assert (d.n_aux, d.n_ctl_constraints, d.n_families) == (16, 40, len(b.families) + 3)
    fams = [(f.first_index, f.count, f.kind, f.degree) for f in d.families[:d.n_families]]
    assert fams[len(b.families):] == [(base, 8, 0, 2), (base + 1, 16, 1, 3), (base + 2, 16, 3, 2)]
    d4 = bpg.ops.air_describe(bpg.ops.air_register(pc.flag_program(ports=4).assemble()))
    assert (d4.n_aux, d4.n_families) == (8, len(b.families) + 20)


def test_set_arguments_are_refused_without_a_device(bpg):
    one = bpg.ops.air_register(pc.flag_program(ports=1).assemble())
    two = bpg.ops.air_register(pc.flag_program(ports=2).assemble())
    cfg = lambda air_id, log_n=5: cases.cfg_for(air_id, log_n, num_queries=6, pow_bits=6)
    A, B, C2 = {"air_id": one, "cfg": cfg(one)}, {"air_id": one, "cfg": cfg(one, 7)}, {"air_id": two, "cfg": cfg(two)}
    nothing = np.zeros(8, dtype=np.uint64)

    def both(tables, links, what):
        # (the prover gets no trace: a statement that passed would be refused for the null pointer, not for `what`)
        for call in (lambda: bpg.ops.stark_prove_table_set(tables, links), lambda: bpg.ops.stark_verify_table_set(tables, links, nothing)):
            with pytest.raises(BpgError) as e:
                call()
            assert e.value.code == -2 and re.search(what, e.value.message), e.value.message

    both([A, C2], [([(0, 0)], (1, 0))], "port 1 of table 1 is in no link")              # an unlinked port
    both([A, B, C2], [([(0, 0)], (1, 0)), ([(0, 0)], (2, 0)), ([(2, 1)], (1, 0))], "named twice")  # a port in two links
    both([A, B], [([(0, 0)], (2, 0))], "names table 2 of 2")                             # a table index out of range
    both([A, B], [([(0, 1)], (1, 0))], "names port 1 of table 0, which has 1")
    both([A] * 9, [([(0, 0)], (1, 0))], "1 .. 8 tables, got 9")                          # 9 tables
    both([A, {"air_id": 4, "cfg": cfg(4)}], [([(0, 0)], (1, 0))], "table 1: air_id 4 .* has no lookup port")
    both([A, {"air_id": cases.register(cases.memory_program()), "cfg": cfg(3)}], [([(0, 0)], (1, 0))], "has no lookup port")
    both([A, B], [([(0, 0)], (1, 0))] * 17, "1 .. 16 links, got 17")
    both([A, {"air_id": one, "cfg": bpg.ops.stark_cfg(5, 9, num_queries=6, pow_bits=6)}], [([(0, 0)], (1, 0))], "table 1: .*8 columns")
    # a well-formed statement gets as far as the container
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_verify_table_set([A, B], [([(0, 0)], (1, 0))], nothing)
    assert e.value.code == -5 and "bad magic" in e.value.message
