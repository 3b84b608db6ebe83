"""Shared by tests/test_air_program_ports.py and tests/test_gpu_air_program_ports.py: programs with lookup ports
("BPGAIRP2", include/bpg.h) made with the Python builder, their witnesses, and the ports' running products over Python
integers -- z[i] = prod_{i' >= i} (1 + f (gamma + sum_j beta^j t_j - 1)) from Builder.evaluate_ports, which shares
nothing with the library's interpreter."""
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
