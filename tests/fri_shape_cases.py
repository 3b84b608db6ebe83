"""The FRI parameter space beyond (cap_height, final_poly_bits) = (4, 5): one table of whole-proof shapes, shared by the host
tests (test_fri_shapes.py) and the GPU tests (test_gpu_fri_shapes.py), and a from-scratch statement of the proof's shape
in Python integers.  Plain data and arithmetic: nothing here calls the oracle or the library.

The expected layer counts and proof lengths in CASES were measured from the oracle (orc_cfg_n_layers, orc_proof_words); the
formula below is held against them by a host test before anything else trusts it."""
from collections import namedtuple

Case = namedtuple("Case", "log_n n_cols n_const deg_pow rate_bits num_queries pow_bits cap_height final_poly_bits")
ARITY_BITS = 4
HEADER_WORDS = 16          # words 9 and 10 of the header: the number of FRI layers, the final polynomial's length

# (case, FRI layers, proof words, what it reaches)
CASES = [
    (Case(4, 8, 0, 1, 1, 5, 6, 0, 0), 1, 631, "root caps; 2^4 folded to a constant; 2-leaf layer tree; fold with log_q = 0"),
    (Case(4, 8, 0, 1, 1, 5, 6, 5, 5), 0, 549, "depth0 = 0: every oracle's cap is its leaf level"),
    (Case(5, 9, 0, 1, 1, 5, 6, 6, 0), 0, 974, "depth0 = 0, ragged width; the cap clause forbids layers although fpb = 0"),
    (Case(8, 16, 0, 1, 1, 7, 8, 0, 0), 2, 1656, "two layers down to one coefficient"),
    (Case(8, 16, 0, 1, 1, 7, 8, 1, 0), 2, 1536, "the last layer's tree is its cap (layer query depth 0)"),
    (Case(8, 16, 0, 1, 1, 7, 8, 8, 0), 0, 3930, "256-entry caps, 256-coefficient final polynomial"),
    (Case(7, 19, 5, 3, 3, 8, 8, 2, 0), 1, 1979, "constants oracle, rate 3; folding stops because d = 3 < arity_bits"),
    (Case(7, 19, 5, 3, 3, 8, 8, 0, 3), 1, 2251, "stops at d == final_poly_bits"),
    (Case(7, 19, 5, 3, 3, 8, 8, 7, 2), 0, 2667, "the cap clause alone decides"),
    (Case(9, 24, 0, 1, 1, 9, 8, 3, 8), 1, 1771, "fpb at its maximum"),
    (Case(12, 16, 0, 1, 1, 9, 8, 0, 0), 3, 3142, "three layers, root caps"),
    (Case(12, 16, 2, 3, 3, 9, 8, 8, 1), 1, 6474, "the cap clause stops after one layer; last layer of 2^11 points"),
    (Case(14, 8, 0, 1, 1, 6, 8, 8, 5), 1, 7059, "final_len = 1024, the longest final polynomial a configuration can have"),
    (Case(13, 8, 0, 1, 1, 6, 8, 7, 8), 1, 3987, "final_len = 512"),
    (Case(11, 12, 0, 1, 1, 6, 8, 4, 3), 2, 1579, "default cap, small fpb"),
]


def case_id(c):
    return "logn%d_C%d_K%d_cap%d_fpb%d" % (c.log_n, c.n_cols, c.n_const, c.cap_height, c.final_poly_bits)


def n_layers(c):
    """FRI with a constant arity of 16.  A polynomial of 2^d coefficients is folded once more only if all three hold:
    it is longer than the final polynomial may be; it has at least 16 coefficients to fold; and the folded codeword, which is
    committed as a tree of 2^(d + rate_bits - 4) leaves of 16 values, has at least as many leaves as a cap has entries."""
    d, layers = c.log_n, 0
    while True:
        longer_than_final = d > c.final_poly_bits
        can_fold = d >= ARITY_BITS
        tree_holds_a_cap = d + c.rate_bits - ARITY_BITS >= c.cap_height
        if not (longer_than_final and can_fold and tree_holds_a_cap):
            return layers
        d -= ARITY_BITS
        layers += 1


def final_len(c):
    return 2 ** (c.log_n - ARITY_BITS * n_layers(c))


def n_aux(c):
    """the synthetic AIR's auxiliary columns: one running product per eight trace columns"""
    return c.n_cols // 8


def layout(c):
    """Word offsets of a proof's sections, its words per query and its length.  A proof is: the header; the caps of the trace,
    auxiliary and quotient trees; the openings at zeta (every column of every oracle), at g * zeta (trace and auxiliary) and
    at 1 (auxiliary), two words each; one cap per FRI layer; the final polynomial's coefficients, two words each; the
    proof-of-work witness; then per query its index, one row of every oracle with a Merkle path of four words per level below
    the cap, and per layer the sixteen values of a leaf (two words each) with its path."""
    cap_words = 4 * 2 ** c.cap_height
    quot = 2 * 2 ** c.rate_bits
    oracle_cols = c.n_const + c.n_cols + n_aux(c) + quot
    n_oracles = 4 if c.n_const else 3
    depth0 = c.log_n + c.rate_bits - c.cap_height
    L = {"cap_words": cap_words, "depth0": depth0, "n_layers": n_layers(c), "final_len": final_len(c)}
    at = HEADER_WORDS
    L["trace_cap"] = at
    at += 3 * cap_words
    at += 2 * oracle_cols + 2 * (c.n_cols + n_aux(c)) + 2 * n_aux(c)
    L["fri_caps"] = at
    at += cap_words * L["n_layers"]
    L["final_poly"] = at
    at += 2 * L["final_len"]
    L["pow"] = at
    at += 1
    L["queries"] = at
    per_query = 1 + oracle_cols + n_oracles * depth0 * 4
    L["layer_depths"] = []
    for layer in range(L["n_layers"]):
        leaves_log = c.log_n + c.rate_bits - ARITY_BITS * (layer + 1)
        L["layer_depths"].append(leaves_log - c.cap_height)
        per_query += 2 * 2 ** ARITY_BITS + 4 * (leaves_log - c.cap_height)
    L["query_words"] = per_query
    L["total"] = at + c.num_queries * per_query
    return L


def proof_words(c):
    return layout(c)["total"]


def flip_words(c):
    """(name, word) of the five places a verifier must notice one flipped bit in: a trace-cap word, a FRI-cap word (where
    there is a layer), a final-polynomial word, the proof-of-work word, and the last word of the last query -- a Merkle path
    word or, where the last tree is its own cap, an opened value."""
    L = layout(c)
    out = [("trace cap", L["trace_cap"] + L["cap_words"] - 3)]
    if L["n_layers"]:
        out.append(("fri cap", L["fri_caps"] + L["cap_words"] * L["n_layers"] - 2))
    out += [("final polynomial", L["final_poly"] + 2 * L["final_len"] - 1), ("pow", L["pow"]), ("last query word", L["total"] - 1)]
    return out


# The L1 chains (two transactions, their aggregation, a block proof) away from the defaults:
# (pg_common base, cap_height, final_poly_bits, the smallest height every table is raised to, or None).
# SMALL_PLONK at cap 6 as pg_common has it cannot be built: its tables 1 and 4 start at 2^5 rows, whose trees of 2^6 leaves
# ARE a cap of 2^6 entries, and a PLONK-shaped circuit that walks a Merkle path of no level is one neither side has
# (air::plonk::layout_ok; a host test holds both sides to refusing it).  The chain runs with those two tables at 2^6 rows.
CHAINS = [("SMALL", 6, 1, None), ("SMALL", 1, 6, None), ("SMALL", 0, 0, None), ("SMALL_PLONK", 3, 0, None), ("SMALL_PLONK", 6, 8, 6)]


def chain_id(ch):
    return "%s_cap%d_fpb%d" % (ch[0], ch[1], ch[2])


def chain_config(ch):
    """-> (the state's configuration as PgState / ProverStateBuilder take it, the seven table heights of its transactions)"""
    import pg_common
    base, cap, fpb, floor = ch
    cfg = dict(getattr(pg_common, base), stark_cap_height=cap, final_poly_bits=fpb)
    log_n = list(pg_common.LOG_N)
    if floor is not None:
        cfg["table_log_lo"] = [max(lo, floor) for lo in cfg["table_log_lo"]]
        log_n = [max(d, floor) for d in log_n]
    return cfg, tuple(log_n)
