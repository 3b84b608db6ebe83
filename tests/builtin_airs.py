"""What the tests know about the built-in table AIRs 1..7, stated once and independently of the library (nothing here
is read from bp_air_describe).  A plain module, not collected.

AIRS[air_id] is one record per AIR: its shape and constraint counts as literals, its named column offsets, its input
generators and row models, the cells whose corruption each constraint family must catch, and the shapes its GPU tests
run.  Each record is built by a function of its own, so that the generators and models read their AIR's column names
unqualified; it ends by naming the locals that are the record's fields.

Below the records: the helpers every AIR test shares (small_cfg, prove, product_verify, oracle_table_proof,
flip_or_set, to_coset_major), the bodies of the three tests tests/test_*_air.py have in common, and the four tests
tests/test_gpu_*_air.py have in common (gpu_tests): those files bind them to their names."""
import ctypes as C
from collections import namedtuple
from types import SimpleNamespace

import numpy as np

from util import coset_major_to_natural, rand_field, to_dev, to_host

P = 0xFFFFFFFF00000001
AIR, FILTER, CHECKER = "air", "lookup filter", "checker"

# One corruption of a valid trace.  Either a cell (col, row, val; val None: flip_or_set's flip) or spoil(trace).
#   fams    the families any of which the trace checker may name for the cell (tests/test_air_check.py takes the
#           entries that have some); None: not among the checker's cases
#   target  AIR: a constraint of the AIR itself; FILTER: a constraint of the table's lookup filter (not in the AIR's own
#           list); CHECKER: a cell only the checker's tests use, no tests/test_*_air.py case
Break = namedtuple("Break", "label col row val spoil fams target")
XOR_40 = "xor 0x40"     # as a cell's val: the cell holds a limb, changed by v ^ 0x40 whatever its value

# what every record has; a record's own fields (its named columns, generators and models) are listed where it is built
FIELDS = ("name n_cols n_aux degree counts trace constraints prefix table in_shape n_families families ctl_families "
          "break_log_n break_trace breaks gpu_seed witness_log_n k5_log_n k5_rng proofs wrong_n_cols note witness_case")


def _record(ns, own):
    """the record of one AIR from its builder's locals: FIELDS and the names in `own`, nothing else"""
    return SimpleNamespace(id=ns["air_id"], **{k: ns[k] for k in (FIELDS + " " + own).split()})


def cell(label, col, row, val=None, fams=None, target=AIR):
    return Break(label, col, row, val, None, fams, target)


def spoiled(label, spoil):
    return Break(label, None, None, None, spoil, None, AIR)


def flip_or_set(trace, col, row, val=None):
    """trace[col, row] = val; val None: the other bit for a bit, another limb value otherwise; XOR_40: another limb value"""
    v = int(trace[col, row])
    if val is XOR_40:
        trace[col, row] = v ^ 0x40
    else:
        trace[col, row] = val if val is not None else ((1 - v) if v <= 1 else v ^ 0x40)


def apply_break(trace, brk):
    if brk.spoil is not None:
        brk.spoil(trace)
    else:
        flip_or_set(trace, brk.col, brk.row, brk.val)


# ---------------------------------------------------------------------------------------------- AIR 1: Keccak-f[1600]


def _keccak():
    air_id, name, n_cols, n_aux, degree = 1, "keccak_f", 2431, 4, 3
    counts = (2826, 10, 11)                                 # AIR constraints, lookup constraints, K5 units
    trace, constraints, prefix = "keccak_trace", "orc_keccak_constraints_base", "F"
    table = 3                                               # its index among a transaction's seven tables
    COL_STEP, COL_A, COL_C, COL_CP, COL_AP, COL_APP, COL_APP0, COL_APPP = 0, 24, 74, 394, 714, 2314, 2364, 2428
    COL_FILTER = 2430

    def in_shape(log_n):
        return (((1 << log_n) + 23) // 24, 25)

    # bp_air_describe's family list: the AIR's own families first, then the table's lookups (csrc/air.hpp, namespace ctl):
    # the filter g (two constraints), the carried input h_c of both challenge sets (fixed on first-round rows, carried on
    # transitions), two filtered running products
    n_families, families = 10, {0: (0, 24, 2, 1), 9: (2776, 50, 1, 2)}
    ctl_families = [(2826, 2, 0, 2), (2828, 1, 0, 2), (2829, 1, 1, 2), (2830, 1, 0, 2), (2831, 1, 1, 2),
                    (2832, 1, 1, 3), (2833, 1, 3, 2), (2834, 1, 1, 3), (2835, 1, 3, 2)]

    def sha3_256_by_hand(permute, msg):
        """The SHA3-256 sponge around a given Keccak-f implementation (rate 136 bytes, domain bits 0x06, final 0x80)."""
        rate = 136
        m = bytearray(msg) + b"\x06"
        m += b"\x00" * (-len(m) % rate)
        m[-1] |= 0x80
        st = np.zeros(25, dtype=np.uint64)
        blocks = []
        for off in range(0, len(m), rate):
            st[:17] ^= np.frombuffer(bytes(m[off:off + rate]), dtype="<u8")
            blocks.append(st.copy())
            st = permute(st)
        return st[:4].astype("<u8").tobytes(), blocks

    def lanes_of(trace, row, col0):
        return np.array([int(trace[col0 + 2 * l, row]) | (int(trace[col0 + 2 * l + 1, row]) << 32) for l in range(25)],
                        dtype=np.uint64)

    # one wrong cell per constraint family: the flag and bit cells are turned over, the limb cells changed by XOR_40.
    # The filter column is zero in the oracle's trace: 0x40 is no bit; 1 is a well-formed bit, on a row that is not a
    # permutation's last round.
    break_log_n = 6

    def break_trace(oracle):
        return oracle.keccak_trace(6, seed=0x5EED)

    breaks = [cell("F1 flags rotate", COL_STEP + 3, 3, fams="F0 F1"), cell("F3/F5 theta", COL_C + 64 * 2 + 17, 9, fams="F3 F5"),
              cell("F3/F4", COL_CP + 64 * 4 + 63, 30, fams="F3 F4"), cell("F4/F5/F6", COL_AP + 64 * 13 + 5, 12, fams="F4 F5 F6"),
              cell("F5/F9 input limb", COL_A + 2 * 7 + 1, 25, XOR_40, fams="F5 F9"),
              cell("F6/F9 chi limb", COL_APP + 2 * 11, 40, XOR_40, fams="F6 F9"),
              cell("F7/F8", COL_APP0 + 31, 2, fams="F7 F8"), cell("F8/F9 iota", COL_APPP + 1, 7, XOR_40, fams="F8 F9"),
              cell("lookup filter is a bit", COL_FILTER, 23, 0x40, target=FILTER),
              cell("lookup filter only on last-round rows", COL_FILTER, 5, 1, target=FILTER)]

    # on the GPU
    gpu_seed = 0x5EED000000000004
    witness_log_n, k5_log_n, k5_rng = [4, 7, 12], [5, 9, 12], 700
    proofs = [(5, 6, 6, 0), (8, 20, 10, 1), (11, 84, 16, 0), (11, 84, 16, 1), (14, 84, 16, 0)]   # (log_n, queries, pow bits, loaded)
    wrong_n_cols = 2432
    note = ("2^14 rows is the S1 Keccak table height (constants.rs:12: the range starts at 14).  The K5 heights spread "
            "the units over grid.y and sum the partial results; the one-pass form (grid.y = 1) runs in the loaded proofs "
            "and in the 2^17 / 2^20-row baseline proofs.")

    def witness_case(oracle, log_n):
        rng = np.random.default_rng(log_n)
        inputs = rng.integers(0, 1 << 64, size=(((1 << log_n) + 23) // 24, 25), dtype=np.uint64)
        inputs[0] = 0                                            # the all-zero state: the Keccak team's known answer

        def spot(got):
            if log_n >= 5:
                assert int(got[COL_APPP, 23]) | (int(got[COL_APPP + 1, 23]) << 32) == 0xF1258F7940E1DDE7
        return inputs, spot
    return _record(locals(), "COL_STEP COL_A COL_C COL_CP COL_AP COL_APP COL_APP0 COL_APPP COL_FILTER sha3_256_by_hand lanes_of")


# ---------------------------------------------------------------------------------------------- AIR 2: logic


def _logic():
    air_id, name, n_cols, n_aux, degree = 2, "logic", 524, 2, 3      # aux: z_0, z_1 of keccak_sponge -> logic
    counts = (524, 5, 8)
    trace, constraints, prefix = "logic_trace", "orc_logic_constraints_base", "L"
    table = 5
    COL_OP, COL_IN0, COL_IN1, COL_RES, COL_FILTER = 0, 3, 259, 515, 523
    OPS = {0: lambda a, b: 0, 1: lambda a, b: a & b, 2: lambda a, b: a | b, 3: lambda a, b: a ^ b}

    def in_shape(log_n):
        return (1 << log_n, 9)

    n_families, families = 4, {0: (0, 3, 0, 2), 1: (3, 1, 0, 2), 2: (4, 512, 0, 2), 3: (516, 8, 0, 3)}
    # the lookup keccak_sponge -> logic: the filter is a bit, two filtered running products
    ctl_families = [(524, 1, 0, 2), (525, 1, 1, 3), (526, 1, 3, 2), (527, 1, 1, 3), (528, 1, 3, 2)]

    def word_of(trace, row, col0):
        return sum(int(trace[col0 + i, row]) << i for i in range(256))

    def result_of(trace, row):
        return sum(int(trace[COL_RES + k, row]) << (32 * k) for k in range(8))

    def random_inputs(n, seed):
        rng = np.random.default_rng(seed)
        inp = rng.integers(0, 1 << 63, size=(n, 9), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 9), dtype=np.uint64)
        inp[:, 0] = rng.integers(0, 4, size=n, dtype=np.uint64)
        return inp

    break_log_n = 6

    def break_trace(oracle):
        inp = random_inputs(1 << 6, 99)
        inp[:, 0] = 1 + (np.arange(1 << 6) % 3)        # every row a real operation: flipping an operand bit changes a result
        inp[11, 0] = 3
        return oracle.logic_trace(6, inputs=inp)

    breaks = [cell("L0 flag not a bit", COL_OP, 3, 2, fams="L0"), cell("L1 two operations / L3", COL_OP + 1, 5, fams="L1 L3"),
              cell("L2 operand bit not a bit", COL_IN0 + 77, 9, 2, fams="L2"), cell("L3 result of limb 6", COL_IN1 + 200, 11, fams="L3"),
              cell("L3 result limb", COL_RES + 4, 20, fams="L3"), cell("lookup filter is a bit", COL_FILTER, 7, 2, target=FILTER)]

    gpu_seed = 0x5EED000000000006
    witness_log_n, k5_log_n, k5_rng = [4, 9, 13], [5, 10, 14], 900
    proofs = [(5, 6, 6, 0), (9, 20, 10, 1), (12, 84, 16, 0), (12, 84, 16, 1), (15, 84, 16, 0)]
    wrong_n_cols = 523
    note = ("2^12 rows is the bottom of the reference's logic range (constants.rs:14).  K5 at 2^5 / 2^10 rows spreads the "
            "eight units and the CTL part over grid.y, 2^14 is closer to one pass.")

    def witness_case(oracle, log_n):
        rng = np.random.default_rng(log_n)
        inputs = rng.integers(0, 1 << 64, size=(1 << log_n, 9), dtype=np.uint64)   # codes: the low two bits of any word

        def spot(got):
            r = 5
            a = sum(int(inputs[r, 1 + w]) << (64 * w) for w in range(4))
            b = sum(int(inputs[r, 5 + w]) << (64 * w) for w in range(4))
            assert result_of(got, r) == OPS[int(inputs[r, 0]) & 3](a, b)
        return inputs, spot
    return _record(locals(), "COL_OP COL_IN0 COL_IN1 COL_RES COL_FILTER OPS word_of result_of random_inputs")


# ---------------------------------------------------------------------------------------------- AIR 3: memory


def _memory():
    air_id, name, n_cols, n_aux, degree = 3, "memory", 45, 2, 3
    counts = (60, 5, 1)
    trace, constraints, prefix = "memory_trace", "orc_memory_constraints_base", "M"
    table = 6
    COL_READ, COL_ADDR, COL_TS, COL_VAL, COL_CHG, COL_GAP, COL_FILTER = 0, 1, 2, 3, 11, 12, 44

    def in_shape(log_n):
        return (1 << log_n, 11)

    n_families, families, ctl_families = 8, {5: (36, 8, 1, 3), 7: (52, 8, 2, 2)}, None

    def random_log(n, seed, n_addr=None):
        """A consistent log: random operations on a few addresses, replayed on a Python dict, then sorted."""
        rng = np.random.default_rng(seed)
        n_addr = n_addr or max(2, n // 5)
        addrs = np.sort(rng.choice(1 << 20, size=n_addr, replace=False))
        mem, ops, ts = {}, [], 0
        for _ in range(n):
            a = int(addrs[rng.integers(0, n_addr)])
            ts += int(rng.integers(1, 1000))
            if rng.integers(0, 2):
                ops.append((1, a, ts, mem.get(a, (0,) * 8)))
            else:
                v = tuple(int(x) for x in rng.integers(0, 1 << 32, size=8))
                mem[a] = v
                ops.append((0, a, ts, v))
        ops.sort(key=lambda o: (o[1], o[2]))
        return np.array([[o[0], o[1], o[2], *o[3]] for o in ops], dtype=np.uint64)

    def check_trace_is_a_memory(t):
        n = t.shape[1]
        assert (t[COL_READ] <= 1).all() and (t[COL_CHG] <= 1).all() and (t[COL_GAP:] <= 1).all()
        mem = {}
        for i in range(n):
            a, rd, v = int(t[COL_ADDR, i]), int(t[COL_READ, i]), tuple(int(x) for x in t[COL_VAL:COL_VAL + 8, i])
            if rd:
                assert v == mem.get(a, (0,) * 8), i
            else:
                mem[a] = v
            if i + 1 < n:
                gap = sum(int(t[COL_GAP + z, i]) << z for z in range(32))
                if int(t[COL_CHG, i]):
                    assert int(t[COL_ADDR, i + 1]) == a + 1 + gap
                else:
                    assert int(t[COL_ADDR, i + 1]) == a and int(t[COL_TS, i + 1]) == int(t[COL_TS, i]) + 1 + gap

    # the cell breaks (M0 .. M4); M5 .. M7 are broken by logs that are not memories (tests/test_memory_air.py)
    break_log_n = 6

    def break_trace(oracle):
        return oracle.memory_trace(6, seed=5)

    breaks = [cell("M0", COL_READ, 3, 2, fams="M0"), cell("M1", COL_CHG, 9, 2, fams="M1"), cell("M2", COL_GAP + 5, 20, 3, fams="M2"),
              cell("M3-M4 flag flipped", COL_CHG, 17, fams="M3 M4")]

    gpu_seed = 0x5EED000000000007
    witness_log_n, k5_log_n, k5_rng = [4, 10, 17], [5, 12, 17], 1100
    proofs = [(5, 6, 6, 0), (9, 20, 10, 1), (13, 84, 16, 0), (17, 84, 16, 1)]
    wrong_n_cols = 48
    note = ("2^17 rows = the S1 memory table (constants.rs:15: the reference's range starts at 17).  The device generator "
            "computes every row independently; the oracle walks the log in order.")

    def witness_case(oracle, log_n):
        """a caller's log up to 2^10 rows (random_log replays it in Python); no spot check: the models are the host tests'"""
        return (random_log(1 << log_n, log_n), None) if log_n <= 10 else None
    return _record(locals(), "COL_READ COL_ADDR COL_TS COL_VAL COL_CHG COL_GAP COL_FILTER random_log check_trace_is_a_memory")


# ---------------------------------------------------------------------------------------------- AIR 4: arithmetic


def _arithmetic():
    air_id, name, n_cols, n_aux, degree = 4, "arithmetic", 309, 1, 2
    counts = (294, 2, 4)
    trace, constraints, prefix = "arithmetic_trace", "orc_arithmetic_constraints_base", "A"
    table = 0
    COL_OP, COL_X, COL_Y, COL_Z, COL_CARRY, COL_RES = 0, 4, 20, 36, 292, 308
    M = 1 << 256

    def in_shape(log_n):
        return (1 << log_n, 9)

    n_families, families, ctl_families = 6, {4: (277, 16, 0, 2)}, None

    def limbs_word(t, r, col0):
        return sum(int(t[col0 + k, r]) << (16 * k) for k in range(16))

    def bits_word(t, r):
        return sum(int(t[COL_Z + i, r]) << i for i in range(256))

    def check_row(t, r, op, x, y):
        assert limbs_word(t, r, COL_X) == x and limbs_word(t, r, COL_Y) == y
        assert [int(t[COL_OP + i, r]) for i in range(4)] == [int(op == i + 1) for i in range(4)]
        z, res = bits_word(t, r), int(t[COL_RES, r])
        if op == 1:
            assert z == (x + y) % M and res == 0 and int(t[COL_CARRY + 15, r]) == (x + y) // M
        elif op == 2:
            assert z == (x - y) % M and res == 0
        elif op == 3:
            assert res == int(x < y) and z == (x - y) % M
        elif op == 4:
            assert res == int(x > y) and z == (y - x) % M
        else:
            assert z == 0 and res == 0 and not t[COL_CARRY:COL_CARRY + 16, r].any()

    def random_inputs(n, seed):
        rng = np.random.default_rng(seed)
        inp = rng.integers(0, 1 << 63, size=(n, 9), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 9), dtype=np.uint64)
        inp[:, 0] = rng.integers(0, 5, size=n, dtype=np.uint64)
        return inp

    def words(v):
        return [(v >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)]

    break_log_n = 6

    def break_trace(oracle):
        inp = random_inputs(1 << 6, 5)
        inp[:, 0] = 1 + (np.arange(1 << 6) % 4)              # every row a real operation
        inp[5, 0] = 2                                        # row 5: sub; setting is_add as well makes two operations
        return oracle.arithmetic_trace(6, inputs=inp)

    breaks = [cell("A0 flag not a bit", COL_OP + 2, 3, 2, fams="A0"), cell("A1 two operations / A4", COL_OP, 5, fams="A1 A4"),
              cell("A2 z bit not a bit", COL_Z + 100, 9, 2, fams="A2"), cell("A3-A4 a carry flipped", COL_CARRY + 7, 11, fams="A3 A4"),
              cell("A4 an x limb changed", COL_X + 3, 13, fams="A4"), cell("A4 the top bit of z", COL_Z + 255, 17, fams="A4"),
              cell("A5 the comparison result", COL_RES, 19, fams="A5")]

    gpu_seed = 0x5EED000000000008
    witness_log_n, k5_log_n, k5_rng = [4, 9, 13], [5, 10, 14], 900
    proofs = [(5, 6, 6, 0), (9, 20, 10, 1), (12, 84, 16, 0), (12, 84, 16, 1), (16, 84, 16, 0)]
    wrong_n_cols = 312
    note = ("2^16 rows is the S1 arithmetic table's height (the reference's range starts there, constants.rs:9).  K5 at "
            "2^5 / 2^10 rows spreads the four units and the CTL part over grid.y, 2^14 is closer to one pass.")

    def witness_case(oracle, log_n):
        rng = np.random.default_rng(log_n)
        inputs = rng.integers(0, 1 << 64, size=(1 << log_n, 9), dtype=np.uint64)
        inputs[:, 0] %= np.uint64(7)                                                 # codes 5 and 6: no operation
        inputs[3, 0] = 3

        def spot(got):
            r = next(i for i in range(1 << log_n) if int(inputs[i, 0]) == 3)         # a comparison, on Python integers
            x = sum(int(inputs[r, 1 + w]) << (64 * w) for w in range(4))
            y = sum(int(inputs[r, 5 + w]) << (64 * w) for w in range(4))
            assert int(got[COL_RES, r]) == int(x < y)
            assert bits_word(got, r) == (x - y) % M
        return inputs, spot
    return _record(locals(), "COL_OP COL_X COL_Y COL_Z COL_CARRY COL_RES M limbs_word bits_word check_row random_inputs words")


# ---------------------------------------------------------------------------------------------- AIR 5: byte packing


def _byte_packing():
    air_id, name, n_cols, n_aux, degree = 5, "byte_packing", 299, 2, 2
    counts = (330, 4, 9)
    trace, constraints, prefix = "byte_packing_trace", "orc_byte_packing_constraints_base", "P"
    table = 1
    COL_READ, COL_LEN, COL_BITS, COL_VAL, COL_ADDR, COL_TS = 0, 1, 33, 289, 297, 298

    def in_shape(log_n):
        return (1 << log_n, 6)

    n_families, families, ctl_families = 6, {5: (322, 8, 0, 2)}, None

    def slots_of(t, r):
        return bytes(sum(int(t[COL_BITS + 8 * s + b, r]) << b for b in range(8)) for s in range(32))

    def check_row(t, r, rd, ln, data):
        assert int(t[COL_READ, r]) == rd
        assert [int(t[COL_LEN + j - 1, r]) for j in range(1, 33)] == [int(ln == j) for j in range(1, 33)]
        s = slots_of(t, r)
        assert s[:ln] == data[:ln] and s[ln:] == bytes(32 - ln)
        value = sum(int(t[COL_VAL + k, r]) << (32 * k) for k in range(8))
        assert value == int.from_bytes(data[:ln], "big")

    def random_inputs(n, seed):
        rng = np.random.default_rng(seed)
        inp = rng.integers(0, 1 << 63, size=(n, 6), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 6), dtype=np.uint64)
        inp[:, 0] = rng.integers(0, 2, size=n, dtype=np.uint64)
        inp[:, 1] = rng.integers(0, 33, size=n, dtype=np.uint64)
        return inp

    break_log_n = 6

    def break_trace(oracle):
        inp = random_inputs(1 << 6, 8)
        inp[:, 1] = 1 + (np.arange(1 << 6) % 32)
        inp[11, 1], inp[17, 1] = 5, 20
        return oracle.byte_packing_trace(6, inputs=inp)

    def two_lengths(t):
        ln = next(j for j in range(1, 33) if t[COL_LEN + j - 1, 5])
        t[COL_LEN + (ln % 32), 5] = 1

    def limb(t):
        t[COL_VAL + 0, 13] = int(t[COL_VAL + 0, 13]) ^ 0x100

    def byte_inside(t):                         # row 17 has len = 20: flipping a bit of slot 3 changes limb 4
        t[COL_BITS + 8 * 3 + 2, 17] = 1 - int(t[COL_BITS + 8 * 3 + 2, 17])

    breaks = [cell("P1 flag not a bit", COL_LEN + 4, 3, 2, fams="P1"), spoiled("P2 two lengths", two_lengths),
              cell("P3 slot bit not a bit", COL_BITS + 70, 9, 2, fams="P3"),
              cell("P4 a byte beyond the length", COL_BITS + 8 * 7 + 1, 11, 1),      # row 11 has len = 5: a byte in slot 7
              spoiled("P5 a value limb", limb), cell("P5 a value limb set", COL_VAL, 13, 0x100, fams="P5", target=CHECKER),
              spoiled("P5 a byte of the sequence", byte_inside), cell("P0 is_read", COL_READ, 2, 3, fams="P0")]

    gpu_seed = 0x5EED000000000009
    witness_log_n, k5_log_n, k5_rng = [4, 9, 13], [5, 10, 14], 900
    proofs = [(5, 6, 6, 0), (9, 84, 16, 1), (9, 84, 16, 0), (12, 84, 16, 1), (14, 84, 16, 0)]
    wrong_n_cols = 300
    note = ("2^9 rows is the S1 byte-packing table's height (the reference's range starts there, constants.rs:10).  K5 at "
            "2^5 / 2^10 rows spreads the nine units and the CTL part over grid.y, 2^14 is closer to one pass.")

    def witness_case(oracle, log_n):
        rng = np.random.default_rng(log_n)
        inputs = rng.integers(0, 1 << 64, size=(1 << log_n, 6), dtype=np.uint64)
        inputs[:, 1] %= np.uint64(40)                                                # lengths above 32 are clipped
        inputs[3, 1] = 7

        def spot(got):
            data = b"".join(int(inputs[3, 2 + w]).to_bytes(8, "little") for w in range(4))
            assert sum(int(got[COL_VAL + k, 3]) << (32 * k) for k in range(8)) == int.from_bytes(data[:7], "big")
        return inputs, spot
    return _record(locals(), "COL_READ COL_LEN COL_BITS COL_VAL COL_ADDR COL_TS slots_of check_row random_inputs")


# ---------------------------------------------------------------------------------------------- AIR 6: Keccak sponge


def _keccak_sponge():
    air_id, name, n_cols, n_aux, degree = 6, "keccak_sponge", 2414, 12, 2   # aux: two products into the Keccak-f table, ten into the logic table
    counts = (2587, 24, 36)
    trace, constraints, prefix = "keccak_sponge_trace", "orc_keccak_sponge_constraints_base", "K"
    table = 4
    COL_FULL, COL_FINAL, COL_LEN, COL_BLOCK, COL_RATE, COL_CAP, COL_XORED, COL_UPDATED = 0, 1, 2, 138, 1226, 2314, 2330, 2364
    MESSAGES = [b"", b"abc", b"q" * 135, b"r" * 136, b"s" * 137, b"The quick brown fox jumps over the lazy dog" * 9]

    def in_shape(log_n):
        return (1 << log_n, 44)

    n_families, families = 11, {8: (2486, 50, 1, 2), 10: (2586, 1, 1, 2)}
    # the twelve looking products (two into the Keccak-f table, ten into the logic table), interleaved transition / last row
    ctl_families = [(2587, 12, 1, 3), (2588, 12, 3, 2)]

    def rows_of(oracle, msgs, log_n):
        rows = np.zeros((1 << log_n, 44), dtype=np.uint64)
        k, digests = 0, []
        for m in msgs:
            d, r = oracle.keccak_sponge_rows(m)
            rows[k:k + len(r)] = r
            k += len(r)
            digests.append(d)
        assert k <= (1 << log_n)
        return rows, k, digests

    def lanes(t, r, col0, n):
        return [int(t[col0 + 2 * l, r]) | (int(t[col0 + 2 * l + 1, r]) << 32) for l in range(n)]

    # Row map of the trace of MESSAGES: 0 "", 1 "abc", 2 q*135, 3-4 r*136, 5-6 s*137, 7-9 the fox (387 bytes: two full
    # blocks and 115 bytes).
    break_log_n = 4

    def break_trace(oracle):
        return oracle.keccak_sponge_trace(4, inputs=rows_of(oracle, MESSAGES, 4)[0])

    def xored(t):
        t[COL_XORED + 11, 8] = int(t[COL_XORED + 11, 8]) ^ 4

    def chain(t):                                # row 8 continues row 7: its state before must be row 7's updated state
        t[COL_RATE + 200, 8] = 1 - int(t[COL_RATE + 200, 8])

    def chain_cap(t):
        t[COL_CAP + 5, 8] = int(t[COL_CAP + 5, 8]) ^ 1

    def full_then_nothing(t):                    # row 9 final -> full: the message would end on a full block
        t[COL_FINAL, 9], t[COL_FULL, 9] = 0, 1

    breaks = [cell("K1 both flags", COL_FINAL, 3, 1), cell("K3 two lengths", COL_LEN + 9, 1, 1), cell("K3 no length", COL_LEN + 3, 1, 0),
              cell("K4 block bit", COL_BLOCK + 50, 7, 2), cell("K5 rate bit", COL_RATE + 70, 8, 2),
              cell("K6 the first pad byte", COL_BLOCK + 8 * 3 + 1, 1, 1),              # "abc": byte 3 must be 0x01
              cell("K6 a zero pad byte", COL_BLOCK + 8 * 60 + 5, 1, 1),               # "abc": byte 60 must be zero
              cell("K6 the last pad bit", COL_BLOCK + 8 * 135 + 7, 1, 0),             # byte 135 must carry 0x80
              spoiled("K7 the xored rate", xored), spoiled("K8 chaining (rate)", chain), spoiled("K8 chaining (capacity)", chain_cap),
              cell("K8 a fresh message", COL_CAP + 2, 5, 7),                          # row 5 starts a message: its state before must be zero
              spoiled("K10 / K3 a message ends on a full block", full_then_nothing), cell("K9 the first row", COL_RATE + 1, 0, 1)]

    gpu_seed = 0x5EED00000000000A
    witness_log_n, k5_log_n, k5_rng = [4, 9, 13], [5, 9, 12], 900
    proofs = [(5, 6, 6, 0), (9, 84, 16, 1), (9, 84, 16, 0), (12, 84, 16, 1)]
    wrong_n_cols = 2416
    note = ("2^9 is the sponge's S1 height (the reference's range starts there, constants.rs:13).  K5 at 2^5 / 2^9 rows "
            "spreads the 36 units and the CTL part over grid.y, 2^12 is closer to one pass.")

    def witness_case(oracle, log_n):
        msgs = (MESSAGES * (1 + (1 << log_n) // 16))[:max(1, (1 << log_n) // 3)]
        rows, k, digests = rows_of(oracle, msgs, log_n)

        def spot(got):    # the first message is empty: its only row's updated state starts with Keccak-256("")
            assert b"".join(x.to_bytes(8, "little") for x in lanes(got, 0, COL_UPDATED, 4)) == digests[0]
        return rows, spot
    return _record(locals(), "COL_FULL COL_FINAL COL_LEN COL_BLOCK COL_RATE COL_CAP COL_XORED COL_UPDATED MESSAGES rows_of lanes")


# ---------------------------------------------------------------------------------------------- AIR 7: multiplication


def _arithmetic_mul():
    air_id, name, n_cols, n_aux, degree = 7, "arithmetic_mul", 1217, 1, 3
    counts = (1218, 2, 8)
    trace, constraints, prefix = "arithmetic_mul_trace", "orc_arithmetic_mul_constraints_base", "U"
    table = 0                                               # the arithmetic table's other half (IR flag 0x4000)
    COL_MUL, COL_X, COL_Y, COL_Z, COL_W, COL_CARRY = 0, 1, 17, 33, 289, 545
    M = 1 << 256

    def in_shape(log_n):
        return (1 << log_n, 9)

    n_families, families, ctl_families = 6, {4: (1185, 32, 0, 3)}, None

    def check_row(t, r, mul, x, y):
        assert int(t[COL_MUL, r]) == mul
        assert sum(int(t[COL_X + k, r]) << (16 * k) for k in range(16)) == x
        assert sum(int(t[COL_Y + k, r]) << (16 * k) for k in range(16)) == y
        z = sum(int(t[COL_Z + i, r]) << i for i in range(256))
        w = sum(int(t[COL_W + i, r]) << i for i in range(256))
        assert z + (w << 256) == (x * y if mul else 0)
        carries = [sum(int(t[COL_CARRY + 21 * k + j, r]) << j for j in range(21)) for k in range(32)]
        assert carries[31] == 0 and (mul or not any(carries))

    def words(v):
        return [(v >> (64 * w)) & 0xFFFFFFFFFFFFFFFF for w in range(4)]

    def random_inputs(n, seed):
        rng = np.random.default_rng(seed)
        inp = rng.integers(0, 1 << 63, size=(n, 9), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=(n, 9), dtype=np.uint64)
        inp[:, 0] = rng.integers(0, 2, size=n, dtype=np.uint64)
        return inp

    break_log_n = 5

    def break_trace(oracle):
        inp = random_inputs(1 << 5, 6)
        inp[:, 0] = 1
        return oracle.arithmetic_mul_trace(5, inputs=inp)

    breaks = [cell("U0 is_mul not a bit", COL_MUL, 3, 2, fams="U0"), cell("U1 z bit not a bit", COL_Z + 77, 5, 2, fams="U1"),
              cell("U2 w bit not a bit", COL_W + 200, 7, 2, fams="U2"), cell("U3 carry bit not a bit", COL_CARRY + 21 * 9 + 4, 9, 2, fams="U3"),
              cell("U4 an x limb", COL_X + 6, 11, fams="U4"), cell("U4 the lowest bit of z", COL_Z + 0, 13, fams="U4"),
              cell("U4 the top bit of w", COL_W + 255, 15, fams="U4"), cell("U4 a carry", COL_CARRY + 21 * 20 + 3, 17, fams="U4"),
              cell("U5 / U4 the top carry", COL_CARRY + 21 * 31, 19, fams="U4 U5")]

    gpu_seed = 0x5EED00000000000B
    witness_log_n, k5_log_n, k5_rng = [4, 9, 13], [5, 10, 14], 900
    proofs = [(5, 6, 6, 0), (9, 20, 10, 1), (12, 84, 16, 0), (12, 84, 16, 1), (14, 84, 16, 0)]
    wrong_n_cols = 1220
    note = "K5 at 2^5 / 2^10 rows spreads the eight units and the CTL part over grid.y, 2^14 is closer to one pass."

    def witness_case(oracle, log_n):
        rng = np.random.default_rng(log_n)
        inputs = rng.integers(0, 1 << 64, size=(1 << log_n, 9), dtype=np.uint64)
        inputs[3, 0] = 1

        def spot(got):
            x = sum(int(inputs[3, 1 + w]) << (64 * w) for w in range(4))
            y = sum(int(inputs[3, 5 + w]) << (64 * w) for w in range(4))
            z = sum(int(got[COL_Z + i, 3]) << i for i in range(256))
            w = sum(int(got[COL_W + i, 3]) << i for i in range(256))
            assert z + (w << 256) == x * y
        return inputs, spot
    return _record(locals(), "COL_MUL COL_X COL_Y COL_Z COL_W COL_CARRY M check_row words random_inputs")


keccak, logic, memory, arithmetic, byte_packing, keccak_sponge, arithmetic_mul = (
    _keccak(), _logic(), _memory(), _arithmetic(), _byte_packing(), _keccak_sponge(), _arithmetic_mul())
AIRS = {a.id: a for a in (keccak, logic, memory, arithmetic, byte_packing, keccak_sponge, arithmetic_mul)}


def table_air(t):
    """the AIR a transaction's table t is proven with when its IR flag is set (table 0: AIR 4; AIR 7 is its other half);
    table 2, the CPU table, has none"""
    return next(a for a in AIRS.values() if a.table == t and a is not arithmetic_mul)


def checker_breaks():
    """(air, column, row, value or None for "xor 1", the families any of which may be named): the cell breaks above
    that the trace checker is held against -- those whose target is the AIR itself (the lookup filters' constraints are
    not the AIR's), and the checker's own"""
    return [(a.id, b.col, b.row, None if b.val is XOR_40 else b.val, b.fams)
            for a in AIRS.values() for b in a.breaks if b.fams is not None]


# ---------------------------------------------------------------------------------------------- shared helpers


def small_cfg(oracle, air, log_n, **kw):
    return oracle.make_cfg(log_n, air.n_cols, air_id=air.id, **dict(dict(num_queries=6, pow_bits=6), **kw))


def prove(oracle, cfg, trace, consts=None):
    """the oracle's table proof of `trace` on a fresh transcript -> (proof, the four lookup challenges, the challenger as
    the verifier needs it: after the caps and the challenges)"""
    cc = oracle.Committed.from_values(consts, cfg.rate_bits, cfg.cap_height) if consts is not None else None
    tc = oracle.Committed.from_values(trace, cfg.rate_bits, cfg.cap_height)
    ch = oracle.PyChallenger()
    if cc is not None:
        ch.observe(cc.cap())
    ch.observe(tc.cap())
    ctl = np.array([ch.challenge() for _ in range(4)], dtype=np.uint64)
    chv = ch.clone()
    return oracle.stark_prove(cfg, trace, ctl, ch, cc, tc), ctl, chv


def product_verify(cfg, air_id, proof, const_cap=None, pub=None):
    """The product's CPU verifier through the C ABI (bp_stark_verify_air; with public inputs bp_stark_verify_air_pub):
    host only, no GPU.  cfg: the oracle's StarkCfg or the product's (the same first ten fields)."""
    import proof_protocol_decoder_amd as pkg
    from proof_protocol_decoder_amd._lib import StarkCfg
    L = pkg.lib()
    pc = StarkCfg(*[getattr(cfg, n) for n, _ in StarkCfg._fields_])
    raw = np.ascontiguousarray(proof, dtype="<u8").tobytes()
    cap = None
    if const_cap is not None:
        cap = np.ascontiguousarray(const_cap, dtype=np.uint64).ctypes.data_as(C.POINTER(C.c_uint64))
    if pub is None:
        return L.bp_stark_verify_air(air_id, C.byref(pc), cap, raw, len(raw))
    return L.bp_stark_verify_air_pub(air_id, C.byref(pc), cap, (C.c_uint64 * 4)(*[int(x) for x in pub]), raw, len(raw))


def oracle_table_proof(oracle, air, log_n, nq, pb, seed):
    """the oracle's proof of the AIR's seeded table -> (cfg, proof, ctl, chv)"""
    cfg = oracle.make_cfg(log_n, air.n_cols, num_queries=nq, pow_bits=pb, air_id=air.id)
    return (cfg,) + prove(oracle, cfg, oracle.air_trace(air.id, log_n, seed=seed))


def to_coset_major(mat, log_n, rate_bits=1):
    """the columns of a natural-order LDE matrix in the coset-major order the device keeps them in"""
    cm = np.empty_like(mat)
    cm[:, coset_major_to_natural(log_n, rate_bits)] = mat
    return cm


# ---------------------------------------------------------------------------------------------- shared test bodies


def check_proof_is_accepted_and_tampering_is_not(oracle, air, log_n, trace):
    """an oracle proof of a valid trace: accepted by the oracle's verifier and by the product's CPU verifier (air.hpp over
    the extension field agrees with the oracle's *_air.c at zeta); one flipped bit is rejected by both"""
    cfg = small_cfg(oracle, air, log_n)
    proof, ctl, chv = prove(oracle, cfg, trace)
    assert int(proof[14]) == air.id
    assert oracle.stark_verify(cfg, proof, ctl, chv.clone(), None) == 0
    assert product_verify(cfg, air.id, proof) == 0
    for word in (20, proof.size // 2, proof.size - 5):
        bad = proof.copy()
        bad[word] ^= np.uint64(1 << 9)
        assert product_verify(cfg, air.id, bad) != 0
        ch = oracle.PyChallenger()
        ch.observe(bad[16:16 + 64])
        c2 = np.array([ch.challenge() for _ in range(4)], dtype=np.uint64)
        assert oracle.stark_verify(cfg, bad, c2, ch, None) != 0
    # a proof claiming another AIR is refused outright
    syn = oracle.make_cfg(log_n, air.n_cols, num_queries=6, pow_bits=6)
    assert oracle.stark_verify(syn, proof, ctl, chv.clone(), None) != 0


def check_break_yields_a_rejected_proof(oracle, air, brk):
    """The prover does not check its witness; the verifier must.  Change ONE thing in a valid trace: the proof made from
    it is rejected by both verifiers at the constraint check."""
    cfg = small_cfg(oracle, air, air.break_log_n)
    trace = air.break_trace(oracle)
    apply_break(trace, brk)
    proof, ctl, chv = prove(oracle, cfg, trace)
    assert oracle.stark_verify(cfg, proof, ctl, chv, None) != 0
    assert product_verify(cfg, air.id, proof) != 0


def check_registry_describes(air):
    """bp_air_describe against the record; returns the family list (first_index, count, kind, degree)"""
    import proof_protocol_decoder_amd as pkg
    pkg.lib()
    d = pkg.ops.air_describe(air.id)
    assert d.name == air.name.encode() and (d.fixed_n_cols, d.n_cols, d.n_aux, d.degree) == (air.n_cols, air.n_cols, air.n_aux, air.degree)
    assert (d.n_air_constraints, d.n_ctl_constraints, d.n_units) == air.counts
    fams = [(f.first_index, f.count, f.kind, f.degree) for f in d.families[:d.n_families]]
    assert sum(c for _, c, _, _ in fams[:air.n_families]) == air.counts[0]
    assert {i: fams[i] for i in air.families} == air.families
    if air.ctl_families is not None:
        assert fams[air.n_families:] == air.ctl_families
    return fams


# ---------------------------------------------------------------------------------------------- shared tests, GPU


def gpu_tests(air):
    """The four GPU tests every built-in AIR has, parametrised by the record's shape lists.  tests/test_gpu_<name>_air.py
    binds them to their names, which with the file's own name are the tests' ids:
        pytestmark, test_witness_matches_oracle, test_quotient_eval_matches_oracle, test_table_proof_bit_exact, \
            test_wrong_shapes_for_the_air_are_refused = gpu_tests(air)"""
    import pytest
    from proof_protocol_decoder_amd._lib import BpgError

    @pytest.mark.parametrize("log_n", air.witness_log_n)
    def test_witness_matches_oracle(bpg, oracle, log_n):
        """the seeded witness through the named entry, then the AIR's own inputs (witness_case) through air_trace and its
        spot check against Python integers or a known answer"""
        seed = air.gpu_seed + log_n
        want = getattr(oracle, air.trace)(log_n, seed=seed)
        got = to_host(getattr(bpg.ops, air.trace)(log_n, seed=seed))
        assert got.shape == want.shape == (air.n_cols, 1 << log_n) and (got == want).all()
        case = air.witness_case(oracle, log_n)
        if case is None:
            return
        inputs, spot = case
        assert inputs.shape == air.in_shape(log_n)
        want = oracle.air_trace(air.id, log_n, inputs=inputs)
        got = to_host(bpg.ops.air_trace(air.id, log_n, inputs=to_dev(inputs)))
        assert (got == want).all()
        if spot is not None:
            spot(got)

    @pytest.mark.parametrize("log_n", air.k5_log_n)
    def test_quotient_eval_matches_oracle(bpg, oracle, log_n):
        """K5 alone: random LDE matrices (the constraints are evaluated on whatever is there -- on the coset the 'bit'
        columns are arbitrary field elements), fixed challenges"""
        rng = np.random.default_rng(air.k5_rng + log_n)
        rows = (1 << log_n) << 1
        trace = rand_field(rng, (air.n_cols, rows))
        aux = rand_field(rng, (air.n_aux, rows))
        ctl, alphas = rand_field(rng, (4,)), rand_field(rng, (2,))
        want = oracle.quotient_values(oracle.make_cfg(log_n, air.n_cols, air_id=air.id), None, trace, aux, ctl, alphas[0], alphas[1])
        got = bpg.ops.quotient_eval(bpg.ops.stark_cfg(log_n, air.n_cols), to_dev(to_coset_major(trace, log_n)),
                                    to_dev(to_coset_major(aux, log_n)), None, ctl, alphas, air_id=air.id)
        assert (to_coset_major(want, log_n) == to_host(got)).all()

    @pytest.mark.parametrize("log_n,nq,pb,loaded", air.proofs)
    def test_table_proof_bit_exact(bpg, oracle, log_n, nq, pb, loaded):
        """prove -> verify, bit-flip rejection, HIP bytes == oracle bytes.  loaded: K5 in ONE pass (all units and the CTL
        part by one workgroup row), as the library runs it while several provers share the device."""
        cfg, want, ctl, chv = oracle_table_proof(oracle, air, log_n, nq, pb, air.gpu_seed)
        pc = bpg.ops.stark_cfg(log_n, air.n_cols, num_queries=nq, pow_bits=pb)
        with bpg.ops.tuned(assume_loaded=loaded):
            got = bpg.ops.stark_prove_air(air.id, pc, air.gpu_seed)
        assert got.shape == want.shape and int(got[14]) == air.id
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, "first mismatch at word %d of %d" % (bad[0], want.size)
        assert oracle.stark_verify(cfg, got, ctl, chv, None) == 0
        assert product_verify(pc, air.id, got) == 0
        flipped = got.copy()
        flipped[got.size // 2] ^= np.uint64(1 << 21)
        assert product_verify(pc, air.id, flipped) != 0

    def test_wrong_shapes_for_the_air_are_refused(bpg):
        for kw in (dict(n_cols=air.wrong_n_cols), dict(n_cols=air.n_cols, n_const=2), dict(n_cols=air.n_cols, deg_pow=3, rate_bits=3)):
            cfg = bpg.ops.stark_cfg(6, kw.pop("n_cols"), num_queries=6, pow_bits=6, **kw)
            with pytest.raises(BpgError, match=air.name):
                bpg.ops.stark_prove_air(air.id, cfg, 1)

    return (pytest.mark.gpu, test_witness_matches_oracle, test_quotient_eval_matches_oracle, test_table_proof_bit_exact,
            test_wrong_shapes_for_the_air_are_refused)
