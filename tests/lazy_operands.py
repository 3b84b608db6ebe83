"""Operands that steer the lazily reduced field forms (csrc/gl.hpp: mul, mul_n, add, sub, mul7; csrc/poseidon.cuh: sbox)
to the UPPER representative r + p of a residue r -- the only place where a lazy value that escapes its contract (reaches
addc / subc / a comparison / a store without a canon) gives a wrong word.  That needs r < 2^32 - 1, which uniformly
random operands meet with probability 2^-32; here it is arranged.  A plain module, not collected: Python integers
throughout, numpy only to hold the matrices, no call into the library or the oracle.

  * mul_model / add_model / sub_model / mul7_model / sbox_model: the device forms step by step, so that a test can
    predict WHICH representative the device returns and count how often a generator reaches the upper one;
  * generic_small_pairs / beta_small_pairs / EDGE: operand pairs;
  * the Poseidon permutation round by round and backwards, and input states whose S-box outputs (or squares) in one
    chosen round are small;
  * plonk_chunk_matrices / plonk_hash_matrices: LDE matrices for AIR 8's quotient whose product trees (the copy
    constraints of csrc/air.hpp eval_chunk_unit) and S-boxes (eval_hash_unit) run through upper representatives, with
    chunk_levels / hash_row_sbox_inputs as the models that say where."""
import os
import re

import numpy as np

from util import rand_field

P = 0xFFFFFFFF00000001
M32 = (1 << 32) - 1
M64 = (1 << 64) - 1
EPS = M32

# the operand edges of test_field_ops_against_big_integers (tests/test_gpu_kernels.py)
EDGE = [0, 1, 2, 7, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, P - 1, P, P + 1, (1 << 63), (1 << 64) - 1,
        (1 << 64) - (1 << 32), (1 << 64) - (1 << 32) - 1, 0xFFFFFFFF00000000, 0x00000000FFFFFFFF,
        0xFFFFFFFEFFFFFFFF, 0x8000000080000000, P - (1 << 32), (1 << 48) + 12345]


# ------------------------------------------------------------------------------------------ the device forms
def mul_model(a, b):
    """gl::mul's device form (csrc/gl.hpp), any u64 x any u64 -> the u64 word it returns.  gl::mul_n<3/4> run the same
    steps on interleaved elements (the same carries, the same two +-EPS corrections), so this is their model too."""
    a0, a1, b0, b1 = a & M32, a >> 32, b & M32, b >> 32
    pp = a0 * b0
    t = a1 * b0 + a0 * b1
    c, m = t >> 64, t & M64                     # M + C 2^64
    q = a1 * b1
    s = (pp >> 32) + (m & M32)
    c1, p1 = s >> 32, s & M32                   # U = (P0, P1 + M0)
    s = (m >> 32) + (q & M32) + c1
    c2, s = s >> 32, s & M32                    # S = M1 + Q0 + c1
    k = (q >> 32) + c                           # K = Q1 + C: fits 32 bits
    v = s * EPS + ((p1 << 32) | (pp & M32))
    c3, v = v >> 64, v & M64
    if c3:
        v = (v + EPS) & M64                     # + EPS on the carry: cannot wrap
    u = v - k - c2
    if u < 0:
        u = (u + (1 << 64) - EPS) & M64         # - EPS on the borrow: cannot borrow
    return u


def add_model(a, b):
    """gl::add: a any u64, b canonical"""
    s = (a + b) & M64
    return (s + EPS) & M64 if s < b else s


def sub_model(a, b):
    """gl::sub: a any u64, b canonical"""
    d = (a - b) & M64
    return (d - EPS) & M64 if a < b else d


def mul7_model(x):
    """gl::mul7: any u64 -> reduced"""
    p = (x & M32) * 7
    m = (x >> 32) * 7 + (p >> 32)
    u = ((m << 32) | (p & M32)) & M64
    t = (u + (m >> 32) * EPS) & M64
    return (t + EPS) & M64 if t < u else t


def sbox_model(x):
    """poseidon::sbox (and sbox_n, the same chain on groups): (x^2, x^4, x^3, x^7) as the device holds them"""
    x2 = mul_model(x, x)
    x4 = mul_model(x2, x2)
    x3 = mul_model(x2, x)
    return x2, x4, x3, mul_model(x3, x4)


def canon(x):
    return x - P if x >= P else x


def inv(x):
    return pow(x, P - 2, P)


def rand_elem(rng, lo=1):
    """one uniform canonical element in [lo, p)"""
    return int(rng.integers(lo, P, dtype=np.uint64))


# ------------------------------------------------------------------------------------------ operand pairs
def generic_small_pairs(rng, n, bound=1 << 16):
    """(a, r / a): generic canonical factors whose product has a residue r in [1, bound)"""
    out = []
    for _ in range(n):
        a, r = rand_elem(rng), int(rng.integers(1, bound))
        out.append((a, r * inv(a) % P))
    return out


def beta_small_pairs(rng, n, bound=16, n_betas=8):
    """(beta, s / beta), s in [1, bound): a challenge times a sigma chosen against it, over a few challenges"""
    betas = [rand_elem(rng) for _ in range(n_betas)]
    out = []
    for i in range(n):
        beta, s = betas[i % n_betas], int(rng.integers(1, bound))
        out.append((beta, s * inv(beta) % P))
    return out


def edge_pairs():
    return [(x, y) for x in EDGE for y in EDGE]


# ------------------------------------------------------------------------------------------ Poseidon in integers
def _parse_rc():
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle", "poseidon_rc.inc")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    rc = [int(h, 16) for h in re.findall(r"0x([0-9a-fA-F]+)ULL", text)]
    assert len(rc) == 360
    return rc


RC = _parse_rc()
_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
MDS = [[_CIRC[(c - r) % 12] + (8 if r == 0 and c == 0 else 0) for c in range(12)] for r in range(12)]
N_ROUNDS = 30


def is_full(rnd):
    return rnd < 4 or rnd >= 26


def _mat_inverse(m):
    n = len(m)
    a = [[v % P for v in row] + [1 if i == j else 0 for j in range(n)] for i, row in enumerate(m)]
    for col in range(n):
        piv = next(r for r in range(col, n) if a[r][col])
        a[col], a[piv] = a[piv], a[col]
        k = inv(a[col][col])
        a[col] = [v * k % P for v in a[col]]
        for r in range(n):
            if r != col and a[r][col]:
                f = a[r][col]
                a[r] = [(v - f * w) % P for v, w in zip(a[r], a[col])]
    return [row[n:] for row in a]


MDS_INV = _mat_inverse(MDS)
SBOX_INV_EXP = pow(7, -1, P - 1)     # 7 d = 1 (mod p - 1)


def _mat_vec(m, v):
    return [sum(a * b for a, b in zip(row, v)) % P for row in m]


def forward_rounds(state):
    """-> (pre, post, out): pre[r] = the state going into round r's S-boxes (round constants added), post[r] = after
    them, out = the permuted state"""
    s = [(int(x) + RC[i]) % P for i, x in enumerate(state)]
    pre, post = [], []
    for r in range(N_ROUNDS):
        pre.append(list(s))
        s = [pow(x, 7, P) if (is_full(r) or i == 0) else x for i, x in enumerate(s)]
        post.append(list(s))
        s = _mat_vec(MDS, s)
        if r + 1 < N_ROUNDS:
            s = [(x + RC[12 * (r + 1) + i]) % P for i, x in enumerate(s)]
    return pre, post, s


def permute(state):
    return forward_rounds(state)[2]


def input_of_pre(rnd, pre):
    """the input state whose round-`rnd` S-box inputs are `pre`"""
    s = list(pre)
    for r in range(rnd, 0, -1):
        s = _mat_vec(MDS_INV, [(x - RC[12 * r + i]) % P for i, x in enumerate(s)])   # post[r - 1]
        s = [pow(x, SBOX_INV_EXP, P) if (is_full(r - 1) or i == 0) else x for i, x in enumerate(s)]  # pre[r - 1]
    return [(x - RC[i]) % P for i, x in enumerate(s)]


def inverse(out):
    post = _mat_vec(MDS_INV, [int(x) % P for x in out])
    r = N_ROUNDS - 1
    return input_of_pre(r, [pow(x, SBOX_INV_EXP, P) if (is_full(r) or i == 0) else x for i, x in enumerate(post)])


def sqrt_mod(a):
    """a square root of a quadratic residue a (Tonelli-Shanks; p - 1 = 2^32 (2^32 - 1))"""
    assert pow(a, (P - 1) // 2, P) == 1
    q, s = (P - 1) >> 32, 32
    c = pow(7, q, P)                    # 7 generates the multiplicative group: a non-residue
    t, r = pow(a, q, P), pow(a, (q + 1) // 2, P)
    while t != 1:
        i, t2 = 0, t
        while t2 != 1:
            t2, i = t2 * t2 % P, i + 1
        b = pow(c, 1 << (s - i - 1), P)
        r, c = r * b % P, b * b % P
        t, s = t * c % P, i
    return r


def seventh_root_of_small(rng, bound=1 << 16):
    """a (generic) x with x^7 in [1, bound)"""
    return pow(int(rng.integers(1, bound)), SBOX_INV_EXP, P)


def root_of_small_square(rng, bound=1 << 16):
    """a (generic) x with x^2 in [2, bound), x^2 no square of an integer below 2^8 (x itself is then not small)"""
    while True:
        r = int(rng.integers(2, bound))
        if int(r ** 0.5) ** 2 != r and pow(r, (P - 1) // 2, P) == 1:
            x = sqrt_mod(r)
            return x if int(rng.integers(0, 2)) else P - x


def _steered_words(rnd):
    return range(12) if is_full(rnd) else range(1)


def state_with_small_sbox_outputs(rnd, rng, bound=1 << 16):
    """an input state of the permutation whose S-box OUTPUTS in round rnd are all in [1, bound): twelve words in a full
    round, word 0 in a partial one (the other eleven words of that round are uniform)"""
    pre = [rand_elem(rng) for _ in range(12)]
    for i in _steered_words(rnd):
        pre[i] = seventh_root_of_small(rng, bound)
    return input_of_pre(rnd, pre)


def state_with_small_squares(rnd, rng, bound=1 << 16):
    """the same with only x^2 small in round rnd's S-boxes: x2 comes out in the upper representative, x4 does not"""
    pre = [rand_elem(rng) for _ in range(12)]
    for i in _steered_words(rnd):
        pre[i] = root_of_small_square(rng, bound)
    return input_of_pre(rnd, pre)


# ------------------------------------------------------------------------------------------ AIR 8: the copy products
# the layout of csrc/air.hpp, namespace plonk
N_COLS, N_CONST, N_AUX = 135, 85, 20
CST_HASH, CST_SIGMA = 4, 5
H_IN, H_OUT, H_FULL1, H_PART, H_FULL2, H_SWAP, H_DELTA = 0, 12, 24, 60, 82, 130, 131
RATE_BITS = 3
N_CHUNKS, N_CLASSES = 10, 12
LEVELS = (1, 2, 3, 4)     # of the lazy product tree; "level" 5 below: the product with Z that closes the chain


def coset_points(log_n):
    """x of natural LDE row i: 7 w^i, w the root of unity of order 8 n"""
    rows = (1 << log_n) << RATE_BITS
    w = pow(7, (P - 1) // rows, P)
    x, out = 7, []
    for _ in range(rows):
        out.append(x)
        x = x * w % P
    return out


def chunk_levels(u, beta, gamma, x, w, sg, prev=None, cur=None):
    """eval_chunk_unit's product tree of chunk u for ONE challenge set, with the device's representatives:
    {"num" / "den": {1: the eight terms, 2: the four pair products, 3: the two halves, 4: the product}} as raw u64 words.
    w, sg: the chunk's eight wires and sigmas (canonical).  With prev, cur (the chunk's two running products Z, canonical)
    also {5: prev num / cur den as gl::mul_n returns it}: the word the closing F::mul4 canonicalises."""
    bkx = canon(mul_model(canon(mul_model(beta, x)), pow(7, 8 * u, P)))      # two canonical products (F::mul4)
    tn, td = [], []
    for i in range(8):
        wg = (w[i] + gamma) % P
        tn.append(add_model(bkx, wg))
        td.append(add_model(mul_model(beta, sg[i]), wg))
        bkx = mul7_model(bkx)
    out = {}
    for side, t in (("num", tn), ("den", td)):
        pair = [mul_model(t[2 * j], t[2 * j + 1]) for j in range(4)]
        half = [mul_model(pair[0], pair[1]), mul_model(pair[2], pair[3])]
        out[side] = {1: t, 2: pair, 3: half, 4: [mul_model(half[0], half[1])]}
        z = prev if side == "num" else cur
        if z is not None:
            out[side][5] = [mul_model(z, out[side][4][0])]
    return out


def z_columns(u, c):
    """the aux columns of (prev, cur) of chunk u, challenge set c; prev of chunk 0 is Z of the NEXT row: None"""
    return (10 * c + u if u else None), 10 * c + (u + 1) % 10


DEN_L1, NUM_L1, CLOSE_NUM, WINDOW, CLOSE_DEN, GENERIC = 0, 4, 8, 9, 10, 11


def chunk_class(row, u):
    """How the (row, chunk) cells are dealt: -> (class, challenge set).  Classes 0..3 steer the denominator's level
    1..4, classes 4..7 the numerator's, CLOSE_NUM and CLOSE_DEN the closing products prev num and cur den (through the
    Z columns), WINDOW both at once (below), GENERIC is left to rand_field.  In this order neighbouring chunks never
    claim the same Z column.  A row's ten chunks run through ten of the twelve classes, in one challenge set or the
    other."""
    return (row + u) % N_CLASSES, ((row + u) // N_CLASSES) % 2


def _small_chain(rng):
    return int(rng.integers(1, 16))


def _terms_with_small_product(rng, level):
    """eight generic terms of which the first 2^(level - 1) multiply to a small residue (never zero)"""
    t = [rand_elem(rng) for _ in range(8)]
    k = 1 << (level - 1)
    prod = 1
    for v in t[:k - 1]:
        prod = prod * v % P
    t[k - 1] = _small_chain(rng) * inv(prod) % P
    return t


def plonk_chunk_matrices(log_n, ctl, rng):
    """(consts [85, rows], trace [135, rows], aux [20, rows]) in natural LDE order for AIR 8's quotient.  Per (row, chunk)
    one level of one side of the copy-product tree of one challenge set is steered to the upper representative
    (chunk_class); the eight terms of a chunk are  td_i = beta sigma_i + w_i + gamma  and  tn_i = beta 7^j x + w_i + gamma:
      level 1  den: sigma_i = s / beta, so beta sigma comes back as s + p, and w_i = t - gamma keeps the sum there;
               num: w_i = t - gamma - beta 7^j x: the lazy sum of two canonical words that add up to t + p
      level 2  the terms generic, the first pair's product small      (generic x generic -> small: upper)
      level 3  the pairs generic, the first half's product small
      level 4  the halves generic, the whole product small
      closing  wires and sigmas generic, Z = s / product: prev num (chunks 1..9), cur den
      window   both halves of the denominator as in level 3 (s1 + p, s2 + p: their product comes back as the LOWER
               s1 s2) and cur = s3, so that cur den is the lower s1 s2 s3 < 2^12, and prev = t / num with t >= 2^12, so
               that prev num comes back as t + p: of all the pairs the closing
               subtraction can meet, the one where gl::subc is wrong by 2^32 - 1 if its operands were left unreduced
               (a < b as words, a - b + p taken without the p that b carries)
    with 1 <= s, s1, s2, s3 < 16.  Everything else is rand_field."""
    rows = (1 << log_n) << RATE_BITS
    consts, trace, aux = rand_field(rng, (N_CONST, rows)), rand_field(rng, (N_COLS, rows)), rand_field(rng, (N_AUX, rows))
    xs = coset_points(log_n)
    ctl = [int(v) for v in ctl]
    for row in range(rows):
        for u in range(N_CHUNKS):
            cls, c = chunk_class(row, u)
            beta, gamma = ctl[2 * c], ctl[2 * c + 1]
            pcol, ccol = z_columns(u, c)
            if cls == GENERIC or beta == 0 or (cls == WINDOW and pcol is None):
                continue
            bkx = beta * xs[row] % P * pow(7, 8 * u, P) % P

            def term(i, den):
                j = 8 * u + i
                other = beta * int(consts[CST_SIGMA + j, row]) if den else bkx * pow(7, i, P)
                return (int(trace[j, row]) + gamma + other) % P

            def steer(den, level, both_halves=False):
                t = _terms_with_small_product(rng, level)
                if both_halves:
                    t[4:] = _terms_with_small_product(rng, level)[:4]
                for i in range(8):
                    trace[8 * u + i, row] = (t[i] - gamma - (term(i, den) - int(trace[8 * u + i, row]) - gamma)) % P

            def product(den):
                prod = 1
                for i in range(8):
                    prod = prod * term(i, den) % P
                return prod

            if cls == WINDOW:
                steer(True, 3, both_halves=True)
                aux[ccol, row] = _small_chain(rng)
                aux[pcol, row] = int(rng.integers(1 << 12, 1 << 16)) * inv(product(False)) % P
            elif cls in (CLOSE_NUM, CLOSE_DEN):
                col = pcol if cls == CLOSE_NUM else ccol
                if col is not None:
                    aux[col, row] = _small_chain(rng) * inv(product(cls == CLOSE_DEN)) % P
            elif cls == DEN_L1:
                for i in range(8):
                    consts[CST_SIGMA + 8 * u + i, row] = _small_chain(rng) * inv(beta) % P
                    trace[8 * u + i, row] = (_small_chain(rng) - gamma) % P
            elif cls == NUM_L1:
                for i in range(8):
                    trace[8 * u + i, row] = (_small_chain(rng) - gamma - bkx * pow(7, i, P)) % P
            else:
                steer(cls < NUM_L1, cls % 4 + 1)
    return consts, trace, aux


def rows_with_upper_words(log_n, ctl, consts, trace, aux):
    """{(side, level): how many rows carry a word >= p at that level of some chunk's tree, in either challenge set};
    level 5: the closing product (chunk 0's numerator has none here: its Z is the next row's)"""
    xs = coset_points(log_n)
    ctl = [int(v) for v in ctl]
    count = {(side, lv): 0 for side in ("num", "den") for lv in LEVELS + (5,)}
    for row in range(len(xs)):
        seen = set()
        for u in range(N_CHUNKS):
            w = [int(trace[8 * u + i, row]) for i in range(8)]
            sg = [int(consts[CST_SIGMA + 8 * u + i, row]) for i in range(8)]
            for c in range(2):
                pcol, ccol = z_columns(u, c)
                tree = chunk_levels(u, ctl[2 * c], ctl[2 * c + 1], xs[row], w, sg,
                                    int(aux[pcol, row]) if pcol is not None else 0, int(aux[ccol, row]))
                for side in ("num", "den"):
                    for lv in LEVELS + (5,):
                        if any(v >= P for v in tree[side][lv]):
                            seen.add((side, lv))
        for k in seen:
            count[k] += 1
    return count


# ------------------------------------------------------------------------------------------ AIR 8: the Poseidon gate
def plonk_hash_matrices(log_n, ctl, rng):
    """The same three matrices with the wires of eval_hash_unit steered.  The gate takes a row's wires at their word: the
    wire blocks 24..59, 60..81, 82..129 ARE the S-box inputs of rounds 1..29, and round 0's are in (+- delta) + rc_0.  Row
    kind = row mod 3:  0: every S-box input a 7th root of a small number (all thirty rounds of the row);  1: every S-box
    input a square root of a small number;  2: rand_field.  q_hash is 1 / 0 / generic by (row // 3) mod 3, the swap
    wire 0 / 1 by (row // 9) mod 2 with delta = swap (in[4 + i] - in[i]), so the swap constraints hold on those rows."""
    rows = (1 << log_n) << RATE_BITS
    consts, trace, aux = rand_field(rng, (N_CONST, rows)), rand_field(rng, (N_COLS, rows)), rand_field(rng, (N_AUX, rows))
    for row in range(rows):
        kind = row % 3
        if kind == 2:
            continue
        q = (row // 3) % 3
        if q < 2:
            consts[CST_HASH, row] = 1 - q
        pick = seventh_root_of_small if kind == 0 else root_of_small_square
        for col in range(H_FULL1, H_SWAP):
            trace[col, row] = pick(rng)
        st = [pick(rng) for _ in range(12)]     # round 0's S-box inputs
        swap = (row // 9) % 2
        trace[H_SWAP, row] = swap
        for i in range(4):
            a, b = (st[i] - RC[i]) % P, (st[4 + i] - RC[4 + i]) % P    # the two digests as they are permuted
            lhs, rhs = (b, a) if swap else (a, b)
            trace[H_IN + i, row], trace[H_IN + 4 + i, row] = lhs, rhs
            trace[H_DELTA + i, row] = (rhs - lhs) % P if swap else 0
            trace[H_IN + 8 + i, row] = (st[8 + i] - RC[8 + i]) % P
    return consts, trace, aux


def hash_row_sbox_inputs(trace, row):
    """[round] -> the S-box inputs eval_hash_unit takes in that round of that row (twelve words, or word 0)"""
    w = [int(trace[c, row]) for c in range(N_COLS)]
    st = [(w[H_IN + i] + w[H_DELTA + i] + RC[i]) % P for i in range(4)]
    st += [(w[H_IN + 4 + i] - w[H_DELTA + i] + RC[4 + i]) % P for i in range(4)]
    st += [(w[H_IN + 8 + i] + RC[8 + i]) % P for i in range(4)]
    out = [st]
    for r in range(1, 4):
        out.append(w[H_FULL1 + 12 * (r - 1):H_FULL1 + 12 * r])
    for r in range(4, 26):
        out.append([w[H_PART + r - 4]])
    for r in range(26, 30):
        out.append(w[H_FULL2 + 12 * (r - 26):H_FULL2 + 12 * (r - 25)])
    return out


# ------------------------------------------------------------------------------------------ small cells (AIR 0..7)
SMALL_ALPHABET = [0, 1, 2, P - 1, P - 2, (1 << 32) - 1, 1 << 32, P - (1 << 32), (1 << 16) - 1]


def small_cells(rng, shape):
    """cells drawn in equal parts from SMALL_ALPHABET and from the limbs below 2^16"""
    pick = rng.integers(0, 2, size=shape)
    alpha = np.array(SMALL_ALPHABET, dtype=np.uint64)[rng.integers(0, len(SMALL_ALPHABET), size=shape)]
    limbs = rng.integers(0, 1 << 16, size=shape, dtype=np.uint64)
    return np.where(pick == 0, alpha, limbs)


# ------------------------------------------------------------------------------------------ FRI fold, stage 0
def fri_stage0_small(vals, rng, bound=1 << 16):
    """vals: [m, 2] extension values in natural order (index i <-> shift w_m^i).  The fold takes, per output point g, the
    sixteen values v_j = vals[g + j m/16]; its first butterfly stage multiplies d_j = v_j - v_(j+8) by w_16^(-j), j < 8.
    Sets v_(j+8) = v_j - s w_16^j with s in [1, bound) per component: every one of those products has the residue s."""
    m = vals.shape[0]
    q = m // 16
    w16 = pow(7, (P - 1) // 16, P)
    out = vals.copy()
    for g in range(q):
        for j in range(8):
            wj = pow(w16, j, P)
            for comp in range(2):
                s = int(rng.integers(1, bound))
                out[g + (j + 8) * q, comp] = (int(out[g + j * q, comp]) - s * wj) % P
    return out
