"""Shared by tests/test_air_program_ports.py and tests/test_gpu_air_program_ports.py: programs with lookup ports
("BPGAIRP2", include/bpg.h) made with the Python builder, their witnesses, and the ports' running products over Python
integers -- z[i] = prod_{i' >= i} (1 + f (gamma + sum_j beta^j t_j - 1)) from Builder.evaluate_ports, which shares
nothing with the library's interpreter.  Below them the table sets the GPU tests prove (product links, the range-check
set of log ports) and the four whose container bytes tests/golden/table_set_digests.json pins."""
import numpy as np

import air_program_cases as cases
from air_program_cases import P
from proof_protocol_decoder_amd.air_program import ALL_ROWS, TRANSITION, Builder

MEM_G = 44


def memory_port_program():
    """cases.memory_program()'s constraints plus AIR 3's lookup as a port: f = loc(44), tuple (is_read, address,
    timestamp, eight value limbs) in ctl::product_term's order."""
    b = cases.memory_program()
    b.port(b.loc(MEM_G), [b.loc(0), b.loc(1), b.loc(2)] + [b.loc(3 + k) for k in range(8)])
    return b


# A small table with a boolean flag column and own constraints that hold on flag_witness(): column 0 the flag (a bit),
# columns 1 .. width the tuple, column width + 1 a counter (next = this + 1), the rest zero.
def flag_program(width=3, n_cols=8, ports=1, degree=None):
    """`ports` ports, each with filter loc(0) and tuple loc(1) .. loc(width) (port k > 0 sends the tuple shifted by k:
    loc(1 + j) + k, so two ports of one table are told apart)"""
    assert width + 2 <= n_cols
    b = Builder(n_cols, degree=degree)
    bit = b.family(1, ALL_ROWS, 2)
    count = b.family(1, TRANSITION, 1)
    zero = b.family(n_cols - width - 2, ALL_ROWS, 1) if n_cols > width + 2 else None
    b.unit()
    f = b.loc(0)
    b.emit(bit, f * f - f)
    b.emit(count, b.nxt(width + 1) - b.loc(width + 1) - 1)
    for j in range(n_cols - width - 2):
        b.emit(zero + j, b.loc(width + 2 + j))
    for k in range(ports):
        b.port(f, [b.loc(1 + j) + k for j in range(width)])
    return b


def flag_witness(log_n, flags, tuples, width=3, n_cols=8, start=5):
    """[n_cols, n] uint64: row i has flag flags[i] and tuple tuples[i] (a sequence of `width` integers)"""
    n = 1 << log_n
    t = np.zeros((n_cols, n), dtype=np.uint64)
    for i in range(n):
        t[0, i] = int(flags[i])
        for j in range(width):
            t[1 + j, i] = int(tuples[i][j]) % P
        t[width + 1, i] = (start + i) % P
    return t


def port_products(b, trace, ctl, consts=None, pub=(0, 0, 0, 0)):
    """[2 * n_ports][n] Python integers: the running products of every port of builder b over the uint64 trace, with
    nxt wrapping at the last row and x = w^i, as the prover's witness kernel sees the rows."""
    n_cols, n = trace.shape
    log_n = n.bit_length() - 1
    w = pow(7, (P - 1) >> log_n, P)
    rows = [[int(v) for v in trace[:, i]] for i in range(n)]
    crow = [[int(v) for v in consts[:, i]] for i in range(n)] if consts is not None else [()] * n
    terms = [[None] * n for _ in range(2 * len(b.ports))]
    x = 1
    for i in range(n):
        for l, (f, t) in enumerate(b.evaluate_ports(rows[i], rows[(i + 1) % n], crow[i], pub, x)):
            for c in range(2):
                beta, gamma = ctl[2 * c], ctl[2 * c + 1]
                v = sum(pow(beta, j, P) * tj for j, tj in enumerate(t)) % P
                terms[2 * l + c][i] = (1 + f * (gamma + v - 1)) % P
        x = x * w % P
    out = []
    for col in terms:
        z, acc = [0] * n, 1
        for i in range(n - 1, -1, -1):
            acc = acc * col[i] % P
            z[i] = acc
        out.append(z)
    return out


# ---------------------------------------------------------------------------------------------- table sets

WIDTH = 3
LINK = [([(0, 0)], (1, 0))]


def field(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def cfg_of(air_id, log_n):
    return cases.cfg_for(air_id, log_n, num_queries=6, pow_bits=6)


def rows_of(log_n, rng, k):
    return sorted(int(v) for v in rng.choice(1 << log_n, size=k, replace=False))


def flagged(log_n, rows, tuples, rng, width=WIDTH, n_cols=8):
    """a flag_witness whose rows `rows` are flagged and hold `tuples`; the other rows hold random tuples, unflagged"""
    n = 1 << log_n
    flags = [0] * n
    body = [[int(v) for v in field(rng, width)] for _ in range(n)]
    for row, tup in zip(rows, tuples):
        flags[row], body[row] = 1, list(tup)
    return flag_witness(log_n, flags, body, width=width, n_cols=n_cols)


def balanced_pair(seed=0xD000, log_a=5, log_b=7):
    """A (2^log_a rows) sends 9 tuples, one of them twice; B (2^log_b rows) exposes a seeded permutation of the 10"""
    rng = np.random.default_rng(seed)
    sent = [[int(v) for v in field(rng, WIDTH)] for _ in range(9)]
    sent.append(list(sent[3]))
    a_rows, b_rows = rows_of(log_a, rng, 10), rows_of(log_b, rng, 10)
    exposed = [sent[k] for k in rng.permutation(10)]
    return flagged(log_a, a_rows, sent, rng), flagged(log_b, b_rows, exposed, rng), a_rows, b_rows


def two_looking_tables(seed=0xD200):
    """(traces of 2^5, 2^6 and 2^7 rows, links): the first two send 6 and 12 tuples, one of them shared; the third exposes
    a seeded permutation of the 18"""
    rng = np.random.default_rng(seed)
    s1 = [[int(v) for v in field(rng, WIDTH)] for _ in range(6)]
    s2 = [[int(v) for v in field(rng, WIDTH)] for _ in range(11)] + [list(s1[0])]
    exposed = [(s1 + s2)[k] for k in rng.permutation(18)]
    traces = [flagged(5, rows_of(5, rng, 6), s1, rng), flagged(6, rows_of(6, rng, 12), s2, rng), flagged(7, rows_of(7, rng, 18), exposed, rng)]
    return traces, [([(0, 0), (1, 0)], (2, 0))]


def memory_readers(bpg):
    """(statement, [reader trace (numpy), memory trace (device)]): a 2^5-row flag table of 11-word tuples that looks nine
    rows of a 2^6-row operation log up in the built-in memory table made from that log"""
    from builtin_airs import memory
    from util import to_dev
    reader = bpg.ops.air_register(flag_program(width=11, n_cols=16).assemble())
    log = memory.random_log(64, 0xE000, n_addr=6)
    rng = np.random.default_rng(0xE001)
    asked = rows_of(6, rng, 9)
    mem = bpg.ops.memory_trace(6, inputs=to_dev(log))
    mem[MEM_G, asked] = 1
    words = [[int(v) for v in log[row]] for row in asked]
    r = flagged(5, rows_of(5, rng, 9), [words[k] for k in rng.permutation(9)], rng, width=11, n_cols=16)
    return [{"air_id": reader, "cfg": cfg_of(reader, 5)}, {"air_id": 3, "cfg": cfg_of(3, 6)}], [r, mem]


LIMBS = 3
SELF_LINK = [([(0, k) for k in range(LIMBS)], (0, LIMBS))]


def range_program(limb_kind_multiplicity=False, n_limbs=LIMBS, looked=True):
    """A table that range-checks its own limbs.  Columns 0 .. n_limbs - 1: the limbs; column 3: which rows send (nothing
    of the table's own constrains it: only the port's f f - f does); column 4: how often the table's constant column
    (0 .. n - 1) is asked for each value; column 5: a counter; columns 6, 7: zero.  Ports 0 .. n_limbs - 1 send a limb each,
    the last port exposes the constant column with the multiplicities as its filter."""
    b = Builder(8, n_const=1 if looked else 0)
    count = b.family(1, TRANSITION, 1)
    zero = b.family(2, ALL_ROWS, 1)
    b.unit()
    b.emit(count, b.nxt(5) - b.loc(5) - 1)
    b.emit(zero, b.loc(6))
    b.emit(zero + 1, b.loc(7))
    for k in range(n_limbs):
        b.log_port(b.loc(3), [b.loc(k)], multiplicity=limb_kind_multiplicity)
    if looked:
        b.log_port(b.loc(4), [b.cst(0)], multiplicity=True)
    return b


def range_witness(log_n, limb_bound, rng, n_limbs=LIMBS):
    """limbs below limb_bound on every row, sent by a seeded two thirds of the rows; multiplicities still zero"""
    n = 1 << log_n
    t = np.zeros((8, n), dtype=np.uint64)
    t[:n_limbs] = rng.integers(0, limb_bound, size=(n_limbs, n), dtype=np.uint64)
    t[3] = (rng.integers(0, 3, size=n) != 0).astype(np.uint64)
    t[5] = np.arange(5, 5 + n, dtype=np.uint64)
    return t


def count_limbs(bpg, t, log_range, out=None, n_limbs=LIMBS):
    from util import to_dev
    return bpg.ops.range_multiplicities(to_dev(t)[:n_limbs], log_range, filter=to_dev(t[3]), out=out)


def self_checked_table(bpg, limb_kind_multiplicity=False, seed=0x1D000):
    """(registered id, trace with honest multiplicities, constants 0 .. 63, the one-table statement)"""
    from util import to_host
    reg = bpg.ops.air_register(range_program(limb_kind_multiplicity).assemble())
    t = range_witness(6, 64, np.random.default_rng(seed))
    t[4] = to_host(count_limbs(bpg, t, 6))
    consts = np.arange(64, dtype=np.uint64).reshape(1, 64)
    return reg, t, consts, [{"air_id": reg, "cfg": cfg_of(reg, 6)}]


def table_set_byte_cases(bpg):
    """{name: (tables with their device traces, links)}: the sets whose "BPGTSET1" containers are pinned byte for byte
    (tools/gen_table_set_golden.py, tests/test_gpu_table_set_bytes.py), the smallest that take every branch of the set
    prover: (a) a product link between tables of 2^4 and 2^6 rows, the second a column slice of stride n + 3 (the pack);
    (b) one table looked up by two others; (c) the log-port range set: constant columns, both ends of the link in one
    table; (d) a run-time table into the built-in memory table.  6 queries and 6 proof-of-work bits as in the GPU tests;
    the proof of work takes the smallest witness, so the bytes follow from the inputs alone."""
    import torch
    from util import to_dev
    flag = bpg.ops.air_register(flag_program().assemble())
    out = {}
    a, b, _, _ = balanced_pair(log_a=4, log_b=6)
    wide = torch.full((8, 64 + 3), -1, dtype=torch.int64, device="cuda")
    wide[:, :64] = to_dev(b)
    out["a_product_link_strided"] = ([{"air_id": flag, "cfg": cfg_of(flag, 4), "trace": to_dev(a)},
                                              {"air_id": flag, "cfg": cfg_of(flag, 6), "trace": wide[:, :64]}], LINK)
    traces, links = two_looking_tables()
    out["b_two_looking_tables"] = ([{"air_id": flag, "cfg": cfg_of(flag, log_n), "trace": to_dev(t)} for log_n, t in zip((5, 6, 7), traces)], links)
    _, t, consts, tables = self_checked_table(bpg)
    out["c_log_range_self_link"] = ([dict(tables[0], trace=to_dev(t), consts=to_dev(consts))], SELF_LINK)
    tables, (r, mem) = memory_readers(bpg)
    out["d_into_built_in_memory"] = ([dict(tables[0], trace=to_dev(r)), dict(tables[1], trace=mem)], LINK)
    return out
