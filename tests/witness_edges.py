"""Edge tables for the seven witness generators (bp_*_trace, AIR 1..7) and the Python-integer row models they are held
against.  A plain module: tests/test_witness_edges.py proves the tables on the CPU (oracle == model, checker, proofs),
tests/test_gpu_witness_edges.py feeds them to the device generators.

A table is (log_n, inputs, labels): `inputs` as bp_*_trace reads them, `labels` one word per input item (a row; for
AIR 1 a permutation):
  valid    within what include/bpg.h documents, and a true statement;
  false    within the documented ranges but not a true statement (memory only);
  outside  outside the documented ranges: the documented behaviour is "what the oracle does".
`Table` adds the AIR, a name, the table's kind (false if any row is, else outside if any row is, else valid) and, for
false and outside MEMORY logs, the rows the model says the AIR must reject.

The models reuse the row checkers of tests/builtin_airs.py and extend them to the columns those leave out (memory:
address_changed and the 32 gap bits; multiplication: the 32 x 21 carry bits; arithmetic: all 16 carries; byte packing:
address and timestamp; Keccak-f and the sponge: every column, from a Keccak-f written here and held against hashlib)."""
from collections import namedtuple

import numpy as np

from builtin_airs import (AIRS, arithmetic as ar, arithmetic_mul as am, byte_packing as bpk, keccak as kk, keccak_sponge as sp,
                          logic as lg, memory as mm)

P = 0xFFFFFFFF00000001
M = 1 << 256
U64 = (1 << 64) - 1
U32 = (1 << 32) - 1
VALID, FALSE, OUTSIDE = "valid", "false", "outside"

Table = namedtuple("Table", "air_id name kind log_n inputs labels violated")
# a 256-bit operand with no structure: every byte different, top bit set
X = int.from_bytes(bytes(range(7, 39)), "little") | (1 << 255)
Y = int.from_bytes(bytes((37 * i + 11) & 0xFF for i in range(32)), "little")


def words(v):
    return [(v >> (64 * w)) & U64 for w in range(4)]


def _table(air_id, name, log_n, rows, labels, violated=None):
    inputs = np.array(rows, dtype=np.uint64)
    assert len(labels) == inputs.shape[0]
    kind = FALSE if FALSE in labels else OUTSIDE if OUTSIDE in labels else VALID
    return Table(air_id, name, kind, log_n, inputs, list(labels), violated)


def _padded(rows, width, log_n):
    """unused rows are padding operations: all-zero input words"""
    assert len(rows) <= 1 << log_n
    return rows + [[0] * width] * ((1 << log_n) - len(rows)), [VALID] * (1 << log_n)


def label_of_row(table, r):
    return table.labels[r // 24 if table.air_id == 1 else r]


# ------------------------------------------------------------------------------------------------ Keccak-f, FIPS 202


def _rot(v, s):
    s %= 64
    return ((v << s) | (v >> (64 - s))) & U64 if s else v


def _round_constants():
    out, r = [], 1
    for _ in range(24):
        rc = 0
        for j in range(7):
            r = ((r << 1) ^ ((r >> 7) * 0x71)) % 256
            if r & 2:
                rc ^= 1 << ((1 << j) - 1)
        out.append(rc)
    return out


def _rotation_offsets():
    off, (x, y) = [0] * 25, (1, 0)
    for t in range(24):
        off[x + 5 * y] = ((t + 1) * (t + 2) // 2) % 64
        x, y = y, (2 * x + 3 * y) % 5
    return off


RC, ROT = _round_constants(), _rotation_offsets()


def keccak_round(a, rnd):
    """one round on 25 lanes (index x + 5y): C, C' = C ^ D, A' = A ^ D, A'' after rho / pi / chi, A'''[0] after iota"""
    c = [a[x] ^ a[x + 5] ^ a[x + 10] ^ a[x + 15] ^ a[x + 20] for x in range(5)]
    d = [c[(x - 1) % 5] ^ _rot(c[(x + 1) % 5], 1) for x in range(5)]
    cp = [c[x] ^ d[x] for x in range(5)]
    ap = [a[l] ^ d[l % 5] for l in range(25)]
    b = [0] * 25
    for x in range(5):
        for y in range(5):
            b[y + 5 * ((2 * x + 3 * y) % 5)] = _rot(ap[x + 5 * y], ROT[x + 5 * y])
    app = [b[x + 5 * y] ^ (~b[(x + 1) % 5 + 5 * y] & U64 & b[(x + 2) % 5 + 5 * y]) for y in range(5) for x in range(5)]
    return c, cp, ap, app, app[0] ^ RC[rnd]


def keccak_f(lanes):
    a = [int(v) for v in lanes]
    for rnd in range(24):
        _, _, _, app, appp0 = keccak_round(a, rnd)
        a = [appp0] + app[1:]
    return a


def _bits(v, n=64):
    return [(v >> z) & 1 for z in range(n)]


def _limbs32(lanes):
    return [x for v in lanes for x in (v & U32, v >> 32)]


def check_keccak(t, inputs):
    """every one of the 2431 columns of every row, from the permutation inputs"""
    n = t.shape[1]
    for p in range((n + 23) // 24):
        a = [int(v) for v in inputs[p]]
        for rnd in range(min(24, n - 24 * p)):
            r = 24 * p + rnd
            c, cp, ap, app, appp0 = keccak_round(a, rnd)
            want = [int(k == rnd) for k in range(24)] + _limbs32(a)
            for x in range(5):
                want += _bits(c[x])
            for x in range(5):
                want += _bits(cp[x])
            for l in range(25):
                want += _bits(ap[l])
            want += _limbs32(app) + _bits(app[0]) + [appp0 & U32, appp0 >> 32, 0]
            got = [int(v) for v in t[:, r]]
            assert len(want) == 2431
            assert got == want, ("keccak", "row", r, "column", next(i for i in range(2431) if got[i] != want[i]))
            assert (kk.lanes_of(t, r, kk.COL_A) == np.array(a, dtype=np.uint64)).all()
            a = [appp0] + app[1:]


def keccak_tables():
    """2^7 rows = five permutations and eight rounds of a sixth: six input states"""
    zero_parity = [(0x9E3779B97F4A7C15 * (l + 1)) & U64 for l in range(20)]
    zero_parity += [zero_parity[x] ^ zero_parity[x + 5] ^ zero_parity[x + 10] ^ zero_parity[x + 15] for x in range(5)]
    assert all(zero_parity[x] ^ zero_parity[x + 5] ^ zero_parity[x + 10] ^ zero_parity[x + 15] ^ zero_parity[x + 20] == 0 for x in range(5))
    states = [[0] * 25, [U64] * 25, [1] + [0] * 24, [0] * 24 + [1 << 63],
              [0xAAAAAAAAAAAAAAAA if l % 2 == 0 else 0x5555555555555555 for l in range(25)], zero_parity]
    return [_table(1, "keccak", 7, states, [VALID] * 6)]


# ------------------------------------------------------------------------------------------------ AIR 2, logic


def check_logic(t, inputs):
    for r in range(t.shape[1]):
        op = int(inputs[r, 0]) & 3                                        # only the low two bits count
        a = sum(int(inputs[r, 1 + w]) << (64 * w) for w in range(4))
        b = sum(int(inputs[r, 5 + w]) << (64 * w) for w in range(4))
        assert lg.word_of(t, r, lg.COL_IN0) == a and lg.word_of(t, r, lg.COL_IN1) == b, r
        assert [int(t[lg.COL_OP + i, r]) for i in range(3)] == [int(op == 1), int(op == 2), int(op == 3)], r
        assert lg.result_of(t, r) == lg.OPS[op](a, b), (r, op)
        assert all(int(t[lg.COL_RES + k, r]) <= U32 for k in range(8)) and int(t[523, r]) == 0, r


def logic_tables():
    rows = []
    for op in (1, 2, 3, 0):
        for a, b in ((0, 0), (M - 1, M - 1), (X, ~X & (M - 1)), (X, X)):
            rows.append([op] + words(a) + words(b))
    for pos in (0, 63, 64, 255):
        for op in (1, 2, 3):
            rows.append([op] + words(1 << pos) + words((1 << pos) | (1 << ((pos + 1) % 256))))
    for op in range(4):
        rows.append([4 + op] + words(X) + words(Y))
        rows.append([(1 << 63) + op] + words(Y) + words(X))
    rows, labels = _padded(rows, 9, 6)
    return [_table(2, "logic", 6, rows, labels)]


# ------------------------------------------------------------------------------------------------ AIR 3, memory


def memory_expected(log):
    """columns 0 .. 44 of every row from the log, on Python integers: the operation reduced mod p, address_changed, the
    32 bits of the gap (the 64-bit difference minus one, modulo 2^32), the filter zero"""
    n = len(log)
    out = []
    for i in range(n):
        r = [int(v) for v in log[i]]
        row = [r[0] & 1] + [v % P for v in r[1:11]]
        if i + 1 < n:
            a_n, t_n = int(log[i + 1][1]), int(log[i + 1][2])
            chg = int(a_n != r[1])
            gap = ((a_n - r[1] - 1) if chg else (t_n - r[2] - 1)) % (1 << 32)
        else:
            chg, gap = 0, 0
        out.append(row + [chg] + _bits(gap, 32) + [0])
    return out


def memory_violated_rows(log):
    """The rows of the log's witness AIR 3 must reject, from AIRS.md section 2's statement of it on the STORED (mod p)
    values: row i answers for the step to row i + 1 (same address when staying; the 32-bit gap equals the difference
    minus one in the field; a read returns the value before it, or zero on a new address), row 0 for a first-row read."""
    e = memory_expected(log)
    bad = set()
    for i in range(len(e) - 1):
        cur, nxt = e[i], e[i + 1]
        chg, gap = cur[mm.COL_CHG], sum(b << z for z, b in enumerate(cur[mm.COL_GAP:mm.COL_GAP + 32]))
        if not chg and nxt[mm.COL_ADDR] != cur[mm.COL_ADDR]:
            bad.add(i)
        step = (nxt[mm.COL_ADDR] - cur[mm.COL_ADDR]) if chg else (nxt[mm.COL_TS] - cur[mm.COL_TS])
        if (step - 1 - gap) % P:
            bad.add(i)
        if nxt[mm.COL_READ] and not chg and nxt[mm.COL_VAL:mm.COL_VAL + 8] != cur[mm.COL_VAL:mm.COL_VAL + 8]:
            bad.add(i)
        if nxt[mm.COL_READ] and chg and any(nxt[mm.COL_VAL:mm.COL_VAL + 8]):
            bad.add(i)
    if e[0][mm.COL_READ] and any(e[0][mm.COL_VAL:mm.COL_VAL + 8]):
        bad.add(0)
    return bad


def check_memory(t, log, is_a_memory):
    want = memory_expected(log)
    for i in range(t.shape[1]):
        got = [int(v) for v in t[:, i]]
        assert got == want[i], ("memory", "row", i, "column", next(c for c in range(45) if got[c] != want[i][c]))
    if is_a_memory:
        mm.check_trace_is_a_memory(t)


TOP = (1 << 32) - 1
ONES8, ZERO8, SOME8 = [U32] * 8, [0] * 8, [0x80000000 + k for k in range(8)]


def _valid_log():
    """16 rows, sorted by (address, timestamp), every value below 2^32"""
    return [
        [0, 0, 0] + ONES8,                       # 0  write limbs 0xFFFFFFFF; timestamp jump 0 -> 2^32 - 1: gap 0xFFFFFFFE
        [1, 0, TOP] + ONES8,                     # 1  read after a write; address 0 -> 1: gap 0
        [1, 1, 5] + ZERO8,                       # 2  a read before any write returns zeros; gap 0x55555555
        [0, 1, 5 + 1 + 0x55555555] + SOME8,      # 3  address 1 -> 2
        [0, 2, 0] + SOME8,                       # 4  gap 0xAAAAAAAA
        [1, 2, 0xAAAAAAAB] + SOME8,              # 5  timestamp + 1: gap 0
        [1, 2, 0xAAAAAAAC] + SOME8,              # 6  address 2 -> 3
        [0, 3, 7] + ONES8,                       # 7  address jump 3 -> 2^32 - 1: gap 0xFFFFFFFB
        [0, TOP, 10] + ONES8,                    # 8
        [1, TOP, 11] + ONES8,
        [0, TOP, 12] + ZERO8,
        [1, TOP, 13] + ZERO8,
        [1, TOP, 14] + ZERO8,
        [0, TOP, 15] + SOME8,
        [1, TOP, TOP - 1] + SOME8,               # 14 gap 0
        [1, TOP, TOP] + SOME8,                   # 15 the last row
    ]


def memory_tables():
    out = [_table(3, "memory-valid", 4, _valid_log(), [VALID] * 16, set())]

    def false_log(name, row, edit):
        log = _valid_log()
        edit(log)
        labels = [FALSE if i == row else VALID for i in range(16)]
        out.append(_table(3, name, 4, log, labels, memory_violated_rows(log)))

    def equal_ts(log): log[6][2] = log[5][2]
    def descending(log): log[7][1] = 1
    def stale(log): log[1][3 + 4] ^= 5
    false_log("memory-equal-timestamps", 6, equal_ts)          # two operations at one time on address 2
    false_log("memory-descending-address", 7, descending)       # 2 -> 1
    false_log("memory-stale-read", 1, stale)                    # a read returns what was not written
    assert [t.violated for t in out[1:]] == [{5}, {6}, {0}]
    log = _valid_log()
    labels = [VALID] * 16
    for i in (8, 9):
        log[i][1] = 1 << 32                                     # an address >= 2^32 (3 -> 2^32: the gap 2^32 - 4 still fits)
    for i in (10, 11):
        log[i][1] = P + 5                                       # an address >= p (stored as 5)
    log[11][2] = log[10][2] + (1 << 32) + 1                     # a timestamp step of 2^32 + 1
    for i in range(12, 16):
        log[i][1] = U64                                         # stored as 2^32 - 2
    for i in range(8, 16):
        labels[i] = OUTSIDE
    out.append(_table(3, "memory-outside", 4, log, labels, memory_violated_rows(log)))
    return out


# ------------------------------------------------------------------------------------------------ AIR 4, arithmetic


def check_arithmetic(t, inputs):
    for r in range(t.shape[1]):
        code = int(inputs[r, 0])
        op = code if code <= 4 else 0                                     # compared as a 64-bit word
        x = sum(int(inputs[r, 1 + w]) << (64 * w) for w in range(4))
        y = sum(int(inputs[r, 5 + w]) << (64 * w) for w in range(4))
        ar.check_row(t, r, op, x, y)
        for k in range(16):                                               # the carry out of every limb
            m = 1 << (16 * (k + 1))
            want = {0: 0, 1: int(x % m + y % m >= m), 2: int(x % m < y % m), 3: int(x % m < y % m), 4: int(y % m < x % m)}[op]
            assert int(t[ar.COL_CARRY + k, r]) == want, (r, k)
        assert (t[ar.COL_Z:, r] <= 1).all() and (t[:ar.COL_X, r] <= 1).all(), r


def arithmetic_tables():
    alt = sum(0xFFFF << (32 * k) for k in range(8))
    pairs = [(0, 0), (M - 1, 1), (M - 1, M - 1), (0, 1), (0, M - 1), (X, X), (X, X + 1), (X + 1, X),
             (X, X ^ (1 << 240)), (X, X ^ 1), (alt, 1)]
    rows = [[op] + words(x) + words(y) for op in (1, 2, 3, 4) for x, y in pairs]
    rows += [[code] + words(X) + words(Y) for code in (5, 6, (1 << 32) + 1, 1 << 63, U64)]
    rows, labels = _padded(rows, 9, 6)
    return [_table(4, "arithmetic", 6, rows, labels)]


# ------------------------------------------------------------------------------------------------ AIR 5, byte packing

BP_LENGTHS = [0, 1, 2, 7, 8, 9, 31, 32, 33, 255]


def check_byte_packing(t, inputs):
    for r in range(t.shape[1]):
        w0, w1 = int(inputs[r, 0]), int(inputs[r, 1])
        data = b"".join(int(inputs[r, 2 + w]).to_bytes(8, "little") for w in range(4))
        bpk.check_row(t, r, w0 & 1, min(w1 & 0xFF, 32), data)
        assert int(t[bpk.COL_ADDR, r]) == (w1 >> 8) & U32 and int(t[bpk.COL_TS, r]) == (w0 >> 8) & U32, r
        assert (t[:bpk.COL_VAL, r] <= 1).all(), r


def byte_packing_tables():
    """the bytes of the sequence are 0xFF / 0x00 / 0x80 then 1, 2, ...; every slot at and beyond len is 0xFF"""
    rows = []
    corners = [(0, 0), (TOP, TOP), (0, TOP), (TOP, 0)]
    for ln in BP_LENGTHS + [32]:
        for pat in range(3):
            k = len(rows)
            if len(rows) == 32:
                break
            real = min(ln, 32)
            seq = [bytes([0xFF] * real), bytes(real), bytes([0x80] + list(range(1, 32)))[:real]][pat]
            data = seq + bytes([0xFF] * (32 - real))
            addr, ts = corners[k % 4]
            high = (0xFFFFFF << 40) if k % 2 else 0                      # bits 40 .. 63 of both words: ignored
            rows.append([(k // 2) & 1 | (ts << 8) | high, ln | (addr << 8) | high] +
                        [int.from_bytes(data[8 * w:8 * w + 8], "little") for w in range(4)])
    assert len(rows) == 32 and {r[0] & 1 for r in rows} == {0, 1}
    return [_table(5, "byte_packing", 5, rows, [VALID] * 32)]


# ------------------------------------------------------------------------------------------------ AIR 6, Keccak sponge

SPONGE_LENGTHS = [0, 1, 135, 136, 137, 271, 272]


def sponge_messages():
    return [bytes((i * 7 + n) & 0xFF for i in range(n)) for n in SPONGE_LENGTHS]


def check_sponge(t, inputs):
    """every one of the 2414 columns of every row from the input words (flags 3 = 0: a padding row; a length of 136 or
    more sets no length flag)"""
    for r in range(t.shape[1]):
        q = [int(v) for v in inputs[r]]
        flags = q[0] & 3
        flags = 0 if flags == 3 else flags
        ln, blk, st = q[1], q[2:19], q[19:44]
        xored = [st[l] ^ blk[l] for l in range(17)]
        out = keccak_f(xored + st[17:]) if flags else [0] * 25
        want = [int(flags == 1), int(flags == 2)] + [int(flags == 2 and ln == j) for j in range(136)]
        for w in blk:
            want += _bits(w)
        for w in st[:17]:
            want += _bits(w)
        want += _limbs32(st[17:]) + _limbs32(xored) + _limbs32(out)
        got = [int(v) for v in t[:, r]]
        assert len(want) == 2414
        assert got == want, ("sponge", "row", r, "column", next(i for i in range(2414) if got[i] != want[i]))


def check_sponge_digests(t, first_rows, msgs):
    """the digest check of tests/test_keccak_sponge_air.py and tests/test_gpu_keccak_sponge_air.py: a message's last row leaves its Keccak-256"""
    from proof_protocol_decoder_amd import compact
    for r0, m in zip(first_rows, msgs):
        last = r0 + len(m) // 136
        out = sp.lanes(t, last, sp.COL_UPDATED, 4)
        assert b"".join(x.to_bytes(8, "little") for x in out) == compact.keccak256(m), len(m)
        assert int(t[sp.COL_LEN + len(m) % 136, last]) == 1 and int(t[sp.COL_LEN:sp.COL_BLOCK, last].sum()) == 1


def sponge_tables():
    """the rows of seven messages back to back, a padding row after each (the fourth with flags = 3), in 2^5 rows; and,
    outside what the header documents, a final row that claims 200 message bytes"""
    from proof_protocol_decoder_amd import proof_gen as pg
    rows, firsts = [], []
    for k, m in enumerate(sponge_messages()):
        firsts.append(len(rows))
        rows += [[int(v) for v in row] for row in pg.keccak256_sponge_rows(m)[1]]
        rows.append([3 if k == 3 else 0] + [0] * 43)
    assert len(rows) == 19
    rows, labels = _padded(rows, 44, 5)
    out = [_table(6, "keccak_sponge", 5, rows, labels)]
    bad, labels = _padded([list(r) for r in rows[:9]], 44, 4)           # the first four messages
    assert bad[2][:2] == [2, 1]
    bad[2][1] = 200                                                      # the final row of the one-byte message
    labels[2] = OUTSIDE
    out.append(_table(6, "keccak_sponge-outside", 4, bad, labels))
    return out, firsts


# ------------------------------------------------------------------------------------------------ AIR 7, multiplication

MAX_CARRY = 0xFFFEF


def mul_carries(x, y):
    """the 32 carries of the schoolbook product over 16-bit limbs, and its 32 product limbs"""
    xs, ys = [(x >> (16 * k)) & 0xFFFF for k in range(16)], [(y >> (16 * k)) & 0xFFFF for k in range(16)]
    carry, carries, limbs = 0, [], []
    for k in range(32):
        s = carry + sum(xs[a] * ys[k - a] for a in range(max(0, k - 15), min(k, 15) + 1))
        limbs.append(s & 0xFFFF)
        carry = s >> 16
        carries.append(carry)
    return carries, limbs


def check_mul(t, inputs):
    # column sums grow with every limb, so (2^256 - 1)^2 has the largest carry of every column: 0xFFFEF at most
    assert max(mul_carries(M - 1, M - 1)[0]) == MAX_CARRY < 1 << 20
    for r in range(t.shape[1]):
        mul = int(inputs[r, 0]) & 1                                       # bit 0 counts
        x = sum(int(inputs[r, 1 + w]) << (64 * w) for w in range(4))
        y = sum(int(inputs[r, 5 + w]) << (64 * w) for w in range(4))
        am.check_row(t, r, mul, x, y)
        carries, limbs = mul_carries(x, y) if mul else ([0] * 32, [0] * 32)
        for k in range(32):
            got = [int(t[am.COL_CARRY + 21 * k + j, r]) for j in range(21)]
            assert got == _bits(carries[k], 21) and got[20] == 0, (r, k)
            pcol = am.COL_Z + 16 * k if k < 16 else am.COL_W + 16 * (k - 16)
            assert [int(t[pcol + j, r]) for j in range(16)] == _bits(limbs[k], 16), (r, k)
        assert (t[am.COL_Z:, r] <= 1).all(), r


def mul_tables():
    every = sum(1 << (16 * k) for k in range(16))
    pairs = [(1, M - 1, M - 1), (1, M - 1, 1), (1, 0, M - 1), (1, (1 << 128) - 1, (1 << 128) + 1), (1, 1 << 255, 2),
             (1, 0xFFFF * every, every), (1, 0xFFFF << 240, 0xABCD << 240), (0, X, Y), (2, X, Y), (3, X, Y), ((1 << 63) + 1, Y, X)]
    rows = [[m] + words(x) + words(y) for m, x, y in pairs]
    rows, labels = _padded(rows, 9, 4)
    return [_table(7, "arithmetic_mul", 4, rows, labels)]


# ------------------------------------------------------------------------------------------------ all of them


def all_tables():
    return (keccak_tables() + logic_tables() + memory_tables() + arithmetic_tables() + byte_packing_tables() + sponge_tables()[0]
            + mul_tables())


def check_model(table, t):
    """the Python-integer model of the table's AIR on a trace of its inputs (the oracle's or the device's)"""
    assert t.shape == (AIRS[table.air_id].n_cols, 1 << table.log_n) and (t < np.uint64(P)).all()
    if table.air_id == 1:
        check_keccak(t, table.inputs)
    elif table.air_id == 2:
        check_logic(t, table.inputs)
    elif table.air_id == 3:
        check_memory(t, table.inputs, table.kind == VALID)
    elif table.air_id == 4:
        check_arithmetic(t, table.inputs)
    elif table.air_id == 5:
        check_byte_packing(t, table.inputs)
    elif table.air_id == 6:
        check_sponge(t, table.inputs)
        if table.kind == VALID:
            check_sponge_digests(t, sponge_tables()[1], sponge_messages())
    else:
        check_mul(t, table.inputs)


def first_difference(table, got, want):
    """None, or "(column, row) label" of the first cell where two traces of the table differ"""
    bad = np.argwhere(got != want)
    if bad.size == 0:
        return None
    c, r = int(bad[0][0]), int(bad[0][1])
    return "first difference at (column %d, row %d), a row labelled %s: %#x != %#x" % (c, r, label_of_row(table, r), int(got[c, r]), int(want[c, r]))


# ------------------------------------------------------------------------------------------------ lookup products
# AIRS.md section 3: with a filter f and the row's tuple compressed by challenge set c = (beta_c, gamma_c),
# v_c = sum_j beta_c^j t_j, the product column is z_c[i] = prod_{i' >= i} (1 + f (gamma_c + v_c - 1)).


def lookup_tuple(air_id, t):
    """the columns of the tuple, each a list of Python integers per row, and the filter"""
    n = t.shape[1]

    def col(c):
        return [int(v) for v in t[c]]

    def limb_of_bits(c0):                                                 # sum_z 2^z bit_z over 32 bit columns
        acc = np.zeros(n, dtype=np.uint64)
        for z in range(32):
            acc += t[c0 + z] << np.uint64(z)
        return [int(v) for v in acc]
    if air_id == 2:     # is_and, is_or, is_xor | 8 limbs of input 0 | of input 1 | of the result; filter g = column 523
        assert (t[3:515] <= 1).all()
        tup = [col(0), col(1), col(2)] + [limb_of_bits(3 + 32 * k) for k in range(8)] + [limb_of_bits(259 + 32 * k) for k in range(8)]
        return tup + [col(515 + k) for k in range(8)], col(523)
    if air_id == 3:     # is_read, address, timestamp, 8 value limbs; filter g = column 44
        return [col(c) for c in range(11)], col(44)
    if air_id == 5:     # is_read, address, timestamp, 8 value limbs; filter = the row has a length
        flags = [int(v) for v in t[1:33].sum(axis=0)]
        return [col(bpk.COL_READ), col(bpk.COL_ADDR), col(bpk.COL_TS)] + [col(bpk.COL_VAL + k) for k in range(8)], flags
    raise ValueError(air_id)


def compress(tup, beta):
    n = len(tup[0])
    v = [0] * n
    for t_j in reversed(tup):                                             # Horner: sum_j beta^j t_j
        v = [(v[i] * beta + t_j[i]) % P for i in range(n)]
    return v


def suffix_products(filt, v, gamma):
    n = len(v)
    z, acc = [0] * n, 1
    for i in range(n - 1, -1, -1):
        acc = acc * ((1 + filt[i] * (gamma + v[i] - 1)) % P) % P
        z[i] = acc
    return z
