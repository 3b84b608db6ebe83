"""What the independent row models of the shipped tables (tests/arithmetic_div_model.py, tests/arithmetic_mod_model.py)
share: 16-bit limbs, the carry bits of r + d + 1, the writers of a row's bit and carry blocks, the model trace, a forged
row, the family of a constraint index and the seeded operand draw.  Like the models it serves it works over Python
integers from the statement in include/bpg.h and AIRS.md section 2 and imports nothing of the package: a model's column
numbers and family sizes stay literals in its own file."""
import random

import numpy as np

P = 0xFFFFFFFF00000001
B = 1 << 16
M256 = (1 << 256) - 1


def limbs(v, n=16):
    return [(v >> (16 * k)) & 0xFFFF for k in range(n)]


def word(ls):
    return sum(int(l) << (16 * k) for k, l in enumerate(ls))


def remainder_chain(w, divisor_limbs):
    """what follows from r, d and z: the carry bits of r + d + 1, limb by limb (all zero under z), and the inverse of the
    sum of the divisor's limbs (zero under z)"""
    rb, db = limbs(w["rb"]), limbs(w["db"])
    borrow, bw = [], 1
    for k in range(16):
        bw = (rb[k] + db[k] + bw) >> 16 if not w["z"] else 0
        borrow.append(bw)
    return {"borrow": borrow, "inv": pow(sum(divisor_limbs), P - 2, P) if not w["z"] else 0}


def put_blocks(row, w, bit_blocks, carry_col, carry_bits):
    """the bit blocks (col, key of the word they spell, bits), bit j of carry k at carry_col + carry_bits k + j, then the
    single cells a forgery writes last; returns the row's cells as Python integers below p"""
    for col, name, n in bit_blocks:
        for j in range(n):
            row[col + j] = (w[name] >> j) & 1
    for k, c in enumerate(w["carry"]):
        for j in range(carry_bits):
            row[carry_col + carry_bits * k + j] = (c >> j) & 1
    for col, v in w.get("poke", {}).items():
        row[col] = v
    return [v % P for v in row]


def trace_of(honest, cells, ops):
    """[n_cols, len(ops)] uint64: the model trace of a list of operations"""
    rows = [cells(honest(*o)) for o in ops]
    return np.array(rows, dtype=np.uint64).T.copy()


def forged(honest, chains, cells, entry):
    """the cells of a catalogue entry's row: (name, the honest operation, the forgery, the families that break)"""
    _, op, forge, _ = entry
    w = honest(*op)
    forge(w)
    poke = w.pop("poke", None)
    chains(w)
    if poke:
        w["poke"] = poke
    return cells(w)


def family_of(families, index):
    for k, (name, count) in enumerate(families):
        if index < count:
            return k, name
        index -= count
    raise ValueError("past the program's own constraints")


def random_ops(n, seed, n_operands, op_choices):
    """seeded operations whose operands have every length from 0 to 256 bits, the op drawn from `op_choices`"""
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        values = [rng.getrandbits(rng.randint(0, 256)) for _ in range(n_operands)]
        out.append((rng.choice(op_choices), *values, rng.randint(0, 1)))
    return out
