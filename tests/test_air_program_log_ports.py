"""Log-derivative lookup ports of run-time AIRs, the part that needs no GPU (csrc/air_program.cpp: the "BPGAIRP3"
validator; bp_air_describe; the builder's log_port; bp_stark_verify_table_set's refusal of a link that mixes product and
log ports).  GPU side: tests/test_gpu_air_program_log_ports.py."""
import re

import numpy as np
import pytest

import air_program_port_cases as pc
from air_program_cases import P
from proof_protocol_decoder_amd import air_program as ap
from proof_protocol_decoder_amd._lib import BpgError
from test_air_program import keccak256


@pytest.fixture(scope="module")
def bpg():
    """the package with its library loaded: nothing here touches a device"""
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    return pkg


def layout(w):
    """word offsets of a "BPGAIRP2" / "BPGAIRP3" program: family table, port table, unit offsets, code"""
    assert int(w[0]) in (ap.MAGIC2, ap.MAGIC3)
    n_fam, n_units, n_ports = int(w[6]), int(w[8]), int(w[10])
    port0 = 11 + 4 * n_fam
    off0 = port0 + n_ports
    return dict(port0=port0, off0=off0, code0=off0 + n_units + n_ports + 1, n_units=n_units, n_ports=n_ports)


def refused(bpg, w, off, what):
    with pytest.raises(BpgError) as e:
        bpg.ops.air_register(w)
    assert e.value.code == -2 and re.search(r"word %d: " % off, e.value.message) and re.search(what, e.value.message), \
        (off, e.value.message)


def families(d):
    return [(f.first_index, f.count, f.kind, f.degree) for f in d.families[:d.n_families]]


def test_a_log_port_program_registers_and_describe_reports_the_five_families(bpg):
    """kind 1 with a quadratic filter (the bit slot has degree 4), kind 2 with the same filter (its zero slot degree 1,
    and 2 deg f is not asked for), in a degree-9 program with a cubic tuple: max(1 + 3, 2) = 4 for the other two"""
    b = pc.flag_program(ports=0, degree=9)
    f = b.loc(0) * b.loc(4)
    t = [b.loc(1), b.loc(2) * b.loc(3) * b.loc(5)]
    assert b.log_port(f, t) == 0 and b.log_port(f, t, multiplicity=True) == 1 and b.port(b.loc(0), [b.loc(1)]) == 2
    w = b.assemble()
    L = layout(w)
    assert int(w[0]) == ap.MAGIC3 == int.from_bytes(b"BPGAIRP3", "little")
    assert [int(v) for v in w[L["port0"]:L["off0"]]] == [2 | 1 << 32, 2 | 2 << 32, 1]
    reg = bpg.ops.air_register(w)
    assert reg == 0x80000000 | int.from_bytes(keccak256(w.astype("<u8").tobytes())[:4], "little") & 0x7FFFFFFF
    d = bpg.ops.air_describe(reg)
    base = b.n_constraints
    assert (d.n_aux, d.n_air_constraints, d.n_ctl_constraints, d.degree) == (6, base, 15, 9)
    fams = families(d)
    assert fams[:len(b.families)] == b.families
    want = [(0, 4), (1, 4), (3, 4), (1, 4), (3, 4)] + [(0, 1), (1, 4), (3, 4), (1, 4), (3, 4)] + [(0, 2), (1, 3), (3, 2), (1, 3), (3, 2)]
    assert fams[len(b.families):] == [(base + k, 1, kind, deg) for k, (kind, deg) in enumerate(want)]
    # a filter of higher degree than 1 + deg t: the running sum's constraints take the filter's degree
    b = pc.flag_program(ports=0, degree=9)
    b.log_port(b.loc(0) * b.loc(4) * b.loc(5), [b.loc(1)], multiplicity=True)
    d = bpg.ops.air_describe(bpg.ops.air_register(b.assemble()))
    assert [(f[2], f[3]) for f in families(d)[-5:]] == [(0, 1), (1, 3), (3, 3), (1, 3), (3, 3)]


def test_the_interleaved_families_of_twenty_own_families_and_two_ports(bpg):
    """20 + 5 * 2 > 24: three interleaved families stand for both ports, with the largest degree among them"""
    b = pc.flag_program(width=1, n_cols=8, ports=0, degree=9)
    for _ in range(17):
        b.emit(b.family(1, 0, 1), b.loc(7))
    assert len(b.families) == 20
    b.log_port(b.loc(0), [b.loc(1) * b.loc(2)])                              # bit 2, sums max(1 + 2, 1) = 3
    b.log_port(b.loc(3) * b.loc(4) * b.loc(5) * b.loc(6), [b.loc(1)], multiplicity=True)   # zero slot 1, sums max(2, 4) = 4
    d = bpg.ops.air_describe(bpg.ops.air_register(b.assemble()))
    base = b.n_constraints
    assert (d.n_aux, d.n_ctl_constraints, d.n_families) == (4, 10, 23)
    assert families(d)[20:] == [(base, 2, 0, 2), (base + 1, 4, 1, 4), (base + 2, 4, 3, 4)]


def test_validator_refuses_bad_log_ports_with_the_word_offset(bpg):
    b = pc.flag_program(ports=0)
    b.log_port(b.loc(0), [b.loc(1)])
    b.log_port(b.loc(2), [b.loc(3), b.loc(1)], multiplicity=True)
    base = b.assemble()
    L = layout(base)
    bpg.ops.air_register(base)

    def mutated(at, value):
        w = base.copy()
        w[at] = np.uint64(value)
        return w

    refused(bpg, mutated(L["port0"], 1 | 3 << 32), L["port0"], "port 0: kind 3")
    refused(bpg, mutated(L["port0"] + 1, 2 | 2 << 32 | 1 << 34), L["port0"] + 1, "port 1: .*bits set above")
    refused(bpg, mutated(L["port0"] + 1, 2 | 2 << 32 | 1 << 63), L["port0"] + 1, "port 1: .*bits set above")
    refused(bpg, mutated(L["port0"], 129 | 1 << 32), L["port0"], "n_tuple = 129")
    refused(bpg, mutated(L["port0"], 1 << 32), L["port0"], "n_tuple = 0")
    # the kind is read from "BPGAIRP3" only: the same word under "BPGAIRP2" is a tuple length out of range
    w = base.copy()
    w[0] = np.uint64(ap.MAGIC2)
    refused(bpg, w, L["port0"], "n_tuple = %d" % (1 | 1 << 32))
    # the kinds are in the bytes, so in the id and the digest
    kind2 = mutated(L["port0"], 1 | 2 << 32)
    assert bpg.ops.air_register(kind2) != bpg.ops.air_register(base)
    assert bpg.ops.air_program_digest(bpg.ops.air_register(kind2)) != bpg.ops.air_program_digest(bpg.ops.air_register(base))


def degree_cases():
    """(name, program degree, filter degree, tuple degree, multiplicity, what the library says)"""
    return [("1 + deg t > degree", 3, 1, 3, False, r"a tuple of degree 3, \(s - s'\) d - f must fit the program's degree 3"),
            ("deg f > degree for kind 2", 3, 4, 1, True, r"a filter of degree 4 and a tuple of degree 1, \(s - s'\) d - f must fit"),
            ("2 deg f > degree for kind 1", 3, 2, 1, False, "a bit filter of degree 2, f f - f must fit the program's degree 3"),
            ("the boundary rule", 3, 1, 2, False, "a tuple of degree 2, the last-row constraint s d - f takes degree 2 in a program of degree 3"),
            ("the boundary rule at degree 9", 9, 9, 1, True, "a filter of degree 9 .* takes degree 8 in a program of degree 9")]


def power(b, col, degree):
    e = b.loc(col)
    for _ in range(degree - 1):
        e = e * b.loc(col)
    return e


@pytest.mark.parametrize("case", degree_cases(), ids=[c[0] for c in degree_cases()])
def test_validator_and_builder_refuse_log_ports_whose_degrees_do_not_fit(bpg, case):
    _, degree, df, dt, mult, what = case
    b = pc.flag_program(ports=1, degree=degree)                  # port 0: a product port that fits
    b.log_port(power(b, 0, df), [b.loc(1), power(b, 2, dt)], multiplicity=mult)
    with pytest.raises(ValueError, match="log port 1: a filter of degree %d and a tuple of degree %d do not fit" % (df, dt)):
        b.assemble()
    w = b.assemble(check_ports=False)
    L = layout(w)
    assert int(w[4]) == degree
    refused(bpg, w, L["off0"] + L["n_units"] + 1, "degree violation: log port 1 has .*" + what)


def test_log_ports_at_the_edge_of_the_degree_rules_register(bpg):
    # kind 2 does not ask for 2 deg f <= degree: a quadratic multiplicity in a degree-3 program
    b = pc.flag_program(ports=0, degree=3)
    b.log_port(b.loc(0) * b.loc(4), [b.loc(1)], multiplicity=True)
    d = bpg.ops.air_describe(bpg.ops.air_register(b.assemble()))
    assert [(f[2], f[3]) for f in families(d)[-5:]] == [(0, 1), (1, 2), (3, 2), (1, 2), (3, 2)]
    # degree 9: a tuple of degree 7 (1 + 7 = 8 = the last-row bound) with a bit filter of degree 4
    b = pc.flag_program(ports=0, degree=9)
    b.log_port(power(b, 0, 4), [power(b, 1, 7)])
    d = bpg.ops.air_describe(bpg.ops.air_register(b.assemble()))
    assert [(f[2], f[3]) for f in families(d)[-5:]] == [(0, 8), (1, 8), (3, 8), (1, 8), (3, 8)]
    # without a declared degree the builder takes what the log port needs
    b = pc.flag_program(ports=0)
    b.log_port(b.loc(0), [b.loc(1) * b.loc(2) * b.loc(3)])
    assert int(b.assemble()[4]) == 4


def test_the_builder_chooses_the_format_by_content_and_p2_bytes_do_not_move(bpg):
    """the ids are those the commit before log ports gave these programs (the builder of that commit assembles the same
    bytes), and they are Keccak-256 of the bytes the builder emits today"""
    assert int(pc.flag_program(ports=0).assemble()[0]) == ap.MAGIC
    before = [(pc.memory_port_program(), 0xB011EEF2), (pc.flag_program(), 0xC831A77A), (pc.flag_program(ports=2), 0xB1A8C264),
              (pc.flag_program(ports=8), 0xA31913F5), (pc.flag_program(width=11, n_cols=16), 0xF33DA7E3),
              (pc.flag_program(ports=1, degree=9), 0xC135C83A)]
    for b, want in before:
        w = b.assemble()
        L = layout(w)
        assert int(w[0]) == ap.MAGIC2 and all(int(v) < 1 << 32 for v in w[L["port0"]:L["off0"]])
        assert 0x80000000 | int.from_bytes(keccak256(w.astype("<u8").tobytes())[:4], "little") & 0x7FFFFFFF == want
        assert bpg.ops.air_register(w) == want
    b = pc.flag_program(ports=2)
    n2 = b.assemble().size
    b.log_port(b.loc(0), [b.loc(1)])
    w3 = b.assemble()
    assert int(w3[0]) == ap.MAGIC3 and w3.size > n2
    # a "BPGAIRP3" program whose ports are all kind 0 is a valid program of its own id, with the product families
    w = pc.flag_program(ports=2).assemble()
    w[0] = np.uint64(ap.MAGIC3)
    reg = bpg.ops.air_register(w)
    assert reg != 0xB1A8C264
    assert families(bpg.ops.air_describe(reg)) == families(bpg.ops.air_describe(0xB1A8C264))


def test_running_columns_over_python_integers():
    """the reference of the GPU tests, on a case small enough to state by hand: one row kept, tuple (5), gamma = 2"""
    b = pc.flag_program(width=1, ports=0)
    b.port(b.loc(0), [b.loc(1)])
    b.log_port(b.loc(0), [b.loc(1)])
    b.log_port(b.loc(2), [b.loc(1)], multiplicity=True)
    t = np.zeros((8, 4), dtype=np.uint64)
    t[0, 2], t[1, 2], t[2] = 1, 5, [0, 3, P - 1, 0]
    t[1, 1] = 9
    ctl = [11, 2, 13, 4]
    cols = b.port_running_columns(t, ctl)
    inv = lambda v: pow(v, P - 2, P)
    assert cols[0] == [7, 7, 7, 1] and cols[1] == [9, 9, 9, 1]              # products: 1 + (gamma + 5 - 1)
    assert cols[2] == [inv(7)] * 3 + [0] and cols[3] == [inv(9)] * 3 + [0]   # sums: 1 / (gamma + 5)
    assert cols[4] == [(3 * inv(11) - inv(7)) % P] * 2 + [(P - inv(7)) % P, 0]
    assert pc.port_products(b, t, ctl)[:2] == cols[:2]
    with pytest.raises(ValueError, match="a pole: port 1, challenge set 0, row 2"):
        b.port_running_columns(t, [11, P - 5, 13, 4])
    t[0, 2] = t[2, 2] = 0                                                    # f = 0 on the pole: the row contributes 0
    assert b.port_running_columns(t, [11, P - 5, 13, 4])[2] == [0, 0, 0, 0]


def test_a_link_that_mixes_product_and_log_ports_is_refused_before_the_container_is_read(bpg):
    import air_program_cases as cases
    b = pc.flag_program(ports=1)
    b.log_port(b.loc(0), [b.loc(1)])
    b.log_port(b.loc(2), [b.loc(3)], multiplicity=True)
    mixed = bpg.ops.air_register(b.assemble())
    cfg = lambda air_id, log_n=5: cases.cfg_for(air_id, log_n, num_queries=6, pow_bits=6)
    M = {"air_id": mixed, "cfg": cfg(mixed)}
    nothing = np.zeros(8, dtype=np.uint64)

    def both(tables, links, code, what):
        for call in (lambda: bpg.ops.stark_prove_table_set(tables, links), lambda: bpg.ops.stark_verify_table_set(tables, links, nothing)):
            with pytest.raises(BpgError) as e:
                call()
            assert e.value.code == code and re.search(what, e.value.message), e.value.message

    # product port 0 of table 0 looked up in log port 2 of table 1
    both([M, M], [([(0, 0)], (1, 2)), ([(0, 1)], (0, 2)), ([(1, 1)], (1, 0))], -2,
         "link 0 mixes product and log ports: port 2 of table 1 is a log port, port 0 of table 0 a product port")
    # a built-in member's ports are product ports
    both([M, {"air_id": 3, "cfg": cfg(3, 6)}], [([(0, 1)], (1, 0)), ([(0, 0)], (0, 2))], -2,
         "link 0 mixes product and log ports: port 0 of table 1 is a product port, port 1 of table 0 a log port")
    # kinds 1 and 2 in one link, both ends in one table, product with product: the statement gets as far as the container
    good = [([(0, 1)], (0, 2)), ([(0, 0)], (1, 0)), ([(1, 1)], (1, 2))]
    with pytest.raises(BpgError) as e:
        bpg.ops.stark_verify_table_set([M, M], good, nothing)
    assert e.value.code == -5 and "bad magic" in e.value.message
