"""AIR 8's Poseidon gate (csrc/air.hpp, plonk::eval_hash_unit), folded two ways over Python integers.

The gate's 118 round constraints are d_k = wire_k - (an affine function of S-box outputs), and every S-box input is a
wire (round 0's: in +- delta + rc_0).  The quotient only uses  sum_k A_k d_k  with A_k = alpha^(T - 1 - idx_k), so the
MDS layers can act on the weights A instead of on the data:

    sum_k A_k d_k  =  sum_k A_k wire_k  -  sum_s C_s sigma_s  -  K

with C (118 words) and K (one word) functions of alpha, the MDS matrix and the round constants alone.  `direct_fold`
is the statement (the predicted states carried through thirty layers, as eval_hash_unit does), `fold_weights` the
transposed recurrences, `transposed_fold` their use; the device's pass (quotient_plonk_hash_kernel) is the latter and
csrc/plonk_hash_fold.hpp makes the same weights.  The five swap constraints (G5) are the same in both forms.

Pairs: the device walks 118 (wire, S-box output) pairs; pair p < 106 is the wire of constraint G4 + p with the S-box
output of that wire, pair 106 + i is output wire i (constraint G4 + 106 + i) with round 0's S-box output i.  The wire
takes the alpha power of its constraint; `pair_table` is the block of the S-box outputs' weights the device reads:
[118][2] = {-C0, -C1} (two challenges), then K0, K1.

Run as a program it checks the two folds against each other on random rows and prints the weights of one alpha."""
import os
import random
import re

P = (1 << 64) - (1 << 32) + 1
MDS_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
# the layout of csrc/air.hpp, namespace plonk
H_IN, H_OUT, H_FULL1, H_PART, H_FULL2, H_SWAP, H_DELTA, H_WIRES = 0, 12, 24, 60, 82, 130, 131, 135
G4, G5, N_CONSTRAINTS, N_CTL_CONSTRAINTS = 90, 208, 213, 22
N_COLS, N_CONST, N_AUX, CST_HASH = 135, 85, 20, 4   # the three matrices of a quotient; the constant column of q_hash
T = N_CONSTRAINTS + N_CTL_CONSTRAINTS   # the length of AIR 8's constraint list: the gate's alpha powers count from its end
N_PAIRS = 118
FOLD_WORDS = 2 * N_PAIRS + 2


def _read_rc():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "proof_protocol_decoder_amd", "csrc", "poseidon_rc.inc")
    with open(path) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    rc = [int(h, 16) for h in re.findall(r"0x([0-9a-fA-F]+)ULL", text)]
    assert len(rc) == 360
    return rc


RC = _read_rc()


def mds_entry(r, c):
    """out[r] = sum_c M[r][c] in[c]  (air.hpp poseidon_mds_entry)"""
    return MDS_CIRC[(c + 12 - r) % 12] + (8 if r == 0 and c == 0 else 0)


def mds(v):
    return [sum(mds_entry(r, c) * v[c] for c in range(12)) % P for r in range(12)]


def mds_t(g):
    """the transposed layer on a weight vector"""
    return [sum(mds_entry(r, c) * g[r] for r in range(12)) % P for c in range(12)]


def sbox(x):
    return pow(x, 7, P)


def rc(r):
    return RC[12 * r:12 * r + 12]


def constraint_index(kind, r=0, i=0):
    if kind == "full1":
        return G4 + 12 * (r - 1) + i
    if kind == "part":
        return G4 + 36 + (r - 4)
    if kind == "full2":
        return G4 + 58 + 12 * (r - 26) + i
    assert kind == "out"
    return G4 + 106 + i


def weight(alpha, idx):
    return pow(alpha, T - 1 - idx, P)


def round0_inputs(w):
    st = [(w[H_IN + i] + w[H_DELTA + i] + RC[i]) % P for i in range(4)]
    st += [(w[H_IN + 4 + i] - w[H_DELTA + i] + RC[4 + i]) % P for i in range(4)]
    st += [(w[H_IN + 8 + i] + RC[8 + i]) % P for i in range(4)]
    return st


def swap_fold(w, alpha):
    """the five constraints of G5: the swap wire is a bit, delta_i = swap (in[4 + i] - in[i])"""
    sw = w[H_SWAP]
    acc = weight(alpha, G5) * (sw * (sw - 1))
    for i in range(4):
        acc += weight(alpha, G5 + 1 + i) * (w[H_DELTA + i] - sw * (w[H_IN + 4 + i] - w[H_IN + i]))
    return acc % P


def direct_fold(w, alpha):
    """sum over the gate's 123 constraints of alpha^(T - 1 - idx) d_idx for one row of 135 wires, the selector left out:
    eval_hash_unit<SELECTOR = false> as written"""
    acc = swap_fold(w, alpha)
    st = round0_inputs(w)

    def check12(col0, idx0):
        nonlocal acc, st
        for i in range(12):
            acc += weight(alpha, idx0 + i) * (w[col0 + i] - st[i])
        st = list(w[col0:col0 + 12])

    for r in range(1, 4):
        st = [(a + b) % P for a, b in zip(mds([sbox(x) for x in st]), rc(r))]
        check12(H_FULL1 + 12 * (r - 1), G4 + 12 * (r - 1))
    st = [(a + b) % P for a, b in zip(mds([sbox(x) for x in st]), rc(4))]
    for r in range(4, 26):
        pv = w[H_PART + r - 4]
        acc += weight(alpha, G4 + 36 + (r - 4)) * (pv - st[0])
        st[0] = sbox(pv)
        st = [(a + b) % P for a, b in zip(mds(st), rc(r + 1))]
    for r in range(26, 30):
        check12(H_FULL2 + 12 * (r - 26), G4 + 58 + 12 * (r - 26))
        st = mds([sbox(x) for x in st])
        if r < 29:
            st = [(a + b) % P for a, b in zip(st, rc(r + 1))]
    check12(H_OUT, G4 + 106)
    return acc % P


def fold_weights(A):
    """A: {constraint index: weight} -> (C, K): C["full", r] twelve weights of round r's S-box outputs (r = 0..3,
    26..29), C["part", r] the weight of partial round r's (r = 4..25), K the constant"""
    a = {r: [A[constraint_index("full1", r, i)] for i in range(12)] for r in range(1, 4)}
    b = {r: A[constraint_index("part", r)] for r in range(4, 26)}
    c = {r: [A[constraint_index("full2", r, i)] for i in range(12)] for r in range(26, 30)}
    o = [A[constraint_index("out", 0, i)] for i in range(12)]
    C, K = {}, 0

    def dot(g, r):
        return sum(x * y for x, y in zip(g, rc(r)))

    for r in range(1, 4):                       # x^(r) = M sigma^(r - 1) + rc_r
        C["full", r - 1] = mds_t(a[r])
        K += dot(a[r], r)
    for r in range(27, 30):
        C["full", r - 1] = mds_t(c[r])
        K += dot(c[r], r)
    C["full", 29] = mds_t(o)                    # the output block: no constants
    g = list(c[26])                             # the partial section, backwards from the state round 26 is checked against
    K += dot(g, 26)
    for r in range(25, 3, -1):
        h = mds_t(g)
        C["part", r] = h[0]
        g = h
        g[0] = b[r]
        K += dot(g, r)
    C["full", 3] = mds_t(g)
    return C, K % P


def pair_of(kind, r=0, i=0):
    """the pair whose S-box output is sigma^(r)_i / sigma_r"""
    if kind == "part":
        return 36 + (r - 4)
    if r == 0:
        return 106 + i
    return 12 * (r - 1) + i if r <= 3 else 58 + 12 * (r - 26) + i


def pair_table(alpha0, alpha1):
    """the device's block: [118][2] = {-C0, -C1}, then K0, K1"""
    out = [0] * FOLD_WORDS
    for j, alpha in enumerate((alpha0, alpha1)):
        A = {idx: weight(alpha, idx) for idx in range(G4, G4 + N_PAIRS)}
        C, K = fold_weights(A)
        for (kind, r), v in C.items():
            if kind == "part":
                out[2 * pair_of("part", r) + j] = -v % P
            else:
                for i in range(12):
                    out[2 * pair_of("full", r, i) + j] = -v[i] % P
        out[2 * N_PAIRS + j] = K
    return out


def pair_values(w):
    """[118] (wire, S-box output) as the device pairs them (canonical here; the device's sigma is any representative)"""
    st = round0_inputs(w)
    wires = list(w[H_FULL1:H_SWAP]) + list(w[H_OUT:H_OUT + 12])
    sig = [sbox(x) for x in w[H_FULL1:H_SWAP]] + [sbox(x) for x in st]
    return list(zip(wires, sig))


def transposed_fold(w, alpha):
    """the same sum from the pair table: 118 S-boxes, 2 x 118 + 5 dot terms, no MDS layer"""
    tab = pair_table(alpha, alpha)
    acc = swap_fold(w, alpha)
    for p, (wire, sig) in enumerate(pair_values(w)):
        acc += weight(alpha, G4 + p) * wire + tab[2 * p] * sig
    return (acc - tab[2 * N_PAIRS]) % P


EDGE_ALPHAS = [0, 1, P - 1, (1 << 32) - 1, P - (1 << 32)]


def main():
    rng = random.Random(8)
    alphas = EDGE_ALPHAS + [rng.randrange(P) for _ in range(3)]
    for alpha in alphas:
        for _ in range(4):
            w = [rng.randrange(P) for _ in range(H_WIRES)]
            assert direct_fold(w, alpha) == transposed_fold(w, alpha), hex(alpha)
    print("direct fold == transposed fold on %d alphas x 4 random rows" % len(alphas))
    tab = pair_table(alphas[-1], alphas[-2])
    print("alpha = (%#x, %#x): K = (%#x, %#x)" % (alphas[-1], alphas[-2], tab[-2], tab[-1]))


if __name__ == "__main__":
    main()
