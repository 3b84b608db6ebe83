"""Cases for the host decisions about a transaction's seven tables (csrc/txn_tables.cpp: the witness form, parse_ir,
plan_traces): an IR, witness data, and what every entry point that takes them must answer.  A plain module:
tests/test_txn_tables.py runs the cases through bp_debug_txn_plan on the CPU, tests/test_gpu_txn_tables.py through the
pre-flight and the prover, tools/gen_txn_tables_golden.py records the proofs of the accepted ones.

A case is (name, flags, log_n, witness, status, match): `flags` the AIR flags of IR word 1 (as the header lists them: the
module reads no table of the library's), `log_n` the seven heights, `witness` None or {table index: items}, where items
is a list of items (lists of words) or Null(n): a null pointer with a count of n; `status` the bp_status every entry
point returns and `match` a substring of its message (None when the status is BP_OK).

Heights lie within CFG: the SMALL configuration with the upper bounds tests/test_gpu_witness_preflight.py raises for its
decoded entry, and the byte-packing table allowed up to 2^8 rows -- the memory table has at least 2^8, so only then can it
be too short for the packing table's two operations per row."""
from collections import namedtuple

from pg_common import IR_MAGIC, LOG_N, SMALL, WIDTH

OK, INVALID, RANGE = 0, -2, -3
Case = namedtuple("Case", "name flags log_n witness status match")
Null = namedtuple("Null", "n")

CFG = dict(SMALL, table_log_hi=[8, 9, 8, 11, 7, 12, 13])
TABLES = ("arithmetic", "byte_packing", "cpu", "keccak", "keccak_sponge", "logic", "memory")
# flag of IR word 1 -> (table index, AIR id, words of a witness item)
FLAGS = {0x100: (3, 1, 25), 0x200: (5, 2, 9), 0x400: (6, 3, 11), 0x800: (0, 4, 9), 0x1000: (1, 5, 6), 0x2000: (4, 6, 44),
         0x4000: (0, 7, 9)}
KECCAK, LOGIC, MEMORY, ARITH, PACKING, SPONGE, MUL = FLAGS
ALL_SIX = KECCAK | LOGIC | MEMORY | ARITH | PACKING | SPONGE
# air::ctl::pairs(): name, looking (table, AIR), looked (table, AIR)
PAIRS = (("keccak_sponge -> keccak_f", (4, 6), (3, 1)), ("byte_packing -> memory", (1, 5), (6, 3)),
         ("keccak_sponge -> logic", (4, 6), (5, 2)))
SEED = 0x7AB1E5


def item_words(t):
    return next(w for tt, _, w in FLAGS.values() if tt == t)


def air_of(flags, t):
    """the AIR the flags select for table t (0: the synthetic one)"""
    return next((a for f, (tt, a, _) in sorted(FLAGS.items()) if tt == t and flags & f), 0)


def ir_words(case):
    """the 25 words of the case's IR; a table proven with an AIR gets that AIR's width"""
    from proof_protocol_decoder_amd import ops
    width = [ops.air_describe(air_of(case.flags, t)).n_cols if air_of(case.flags, t) else WIDTH[t] for t in range(7)]
    return [IR_MAGIC, 1 | case.flags, 7, 0, 100, 121, 1, 2, 3, 4, SEED, *case.log_n, *width]


def witness_struct(pg, case):
    """(pg.TxnWitness or None, the arrays it points into) of a case, null pointers included"""
    import ctypes as C
    if case.witness is None:
        return None, []
    w, keep = pg.TxnWitness(), []
    for t, items in case.witness.items():
        ptr_f, n_f, has_f, words = pg.WITNESS_FIELDS[t]
        assert words == item_words(t)
        if isinstance(items, Null):
            setattr(w, n_f, items.n)
        else:
            flat = [int(x) for it in items for x in it]
            a = (C.c_uint64 * max(len(flat), 1))(*flat)
            keep.append(a)
            setattr(w, ptr_f, C.cast(a, C.c_void_p))
            setattr(w, n_f, len(items))
        setattr(w, has_f, 1)
    return w, keep


def zeros(t, n):
    """n items of all-zero words: padding operations, and for Keccak permutations of the zero state"""
    return [[0] * item_words(t)] * n


def _logs(**kw):
    ln = list(LOG_N)
    for name, v in kw.items():
        ln[TABLES.index(name)] = v
    return tuple(ln)


def _cases():
    c = []

    def add(name, flags, witness=None, status=OK, match=None, **logs):
        c.append(Case(name, flags, _logs(**logs), witness, status, match))
    # ---- accepted
    add("no_flag", 0)
    for f, (t, air, _) in sorted(FLAGS.items()):
        add("alone_air%d" % air, f)
    add("six_together", ALL_SIX)
    add("mul_with_the_other_five", ALL_SIX ^ ARITH | MUL)
    add("pair_sponge_keccak_seeded", SPONGE | KECCAK)
    add("pair_packing_memory_seeded", PACKING | MEMORY)
    add("pair_sponge_logic_seeded", SPONGE | LOGIC)
    add("arithmetic_given_under_mul", MUL, {0: []})
    add("keccak_full", KECCAK, {3: zeros(3, 6)}, keccak=7)                       # ceil(128 / 24) = 6
    # sponge 2^5 rows, logic 2^6: min(32, 64 // 5) = 12 rows are covered, 60 XORs first, room for 4 operations
    add("logic_fits_behind_the_xors", SPONGE | LOGIC, {5: zeros(5, 4)}, keccak_sponge=5, logic=6)
    # ---- refused
    for t in (0, 1, 3, 4, 5, 6):
        add("flag_clear_%s" % TABLES[t], 0, {t: []}, INVALID, "witness data for table %s needs an IR whose" % TABLES[t])
    add("keccak_one_too_many", KECCAK, {3: zeros(3, 7)}, RANGE, "7 witness items do not fit table keccak of 2^7 rows (24 rows per", keccak=7)
    add("logic_one_too_many_rows", LOGIC, {5: zeros(5, 65)}, RANGE, "65 witness items do not fit table logic of 2^6 rows", logic=6)
    add("null_data", MEMORY, {6: Null(3)}, INVALID, "null data for table memory")
    add("two_arithmetic_airs", ARITH | MUL, None, INVALID, "the arithmetic table is proven by ONE AIR (flags 0x800 and 0x4000")
    add("unknown_flag", 0x8000, None, INVALID, "IR: bad magic/version")
    add("packing_given_memory_not", PACKING | MEMORY, {1: []}, INVALID, "byte-packing sequences are given but the memory log is not")
    add("memory_given_packing_not", PACKING | MEMORY, {6: []}, INVALID, "the memory log is given but the byte-packing sequences are not")
    add("perms_given_sponge_not", KECCAK | SPONGE, {3: []}, INVALID, "Keccak-f permutations are given but the sponge rows are not")
    add("memory_too_short", PACKING | MEMORY, None, INVALID, "the memory table (2^8 rows) cannot hold the operations of the "
        "byte-packing table (2^8 rows)", byte_packing=8, memory=8)
    add("logic_one_too_many_behind_the_xors", SPONGE | LOGIC, {5: zeros(5, 5)}, INVALID,
        "holds the sponge table's 60 XORs first: room for 4 operations, 5 given", keccak_sponge=5, logic=6)
    return c


CASES = _cases()
ACCEPTED = [c for c in CASES if c.status == OK]
REFUSED = [c for c in CASES if c.status != OK]
FULL_PROOF = "six_together"   # the case whose whole transaction proof is recorded too


def decoded_case():
    """the decoded entry of tests/test_gpu_witness_preflight.py with its own witness: (case, its IR words)"""
    import struct
    import test_decoding as td
    from proof_protocol_decoder_amd import decoding
    from proof_protocol_decoder_amd.block_driver import irs_from_generation_inputs
    m = td.fresh_model()
    infos = [t for t, _ in td.block(m)]
    other = decoding.OtherBlockData(decoding.BlockLevelData(b"meta", b"hashes", [(td.B, 100)]), b"\x22" * 32)
    gis = decoding.into_txn_proof_gen_ir(td.make_trace(m, infos, hash_out_storage_of=(td.E,)), other)
    irs = irs_from_generation_inputs(gis, 24, LOG_N, WIDTH, keccak_air=True, keccak_trie_nodes=True, memory_air=True,
                                     byte_packing_air=True, keccak_sponge_air=True)
    ir = next(ir for g, ir in zip(gis, irs) if g.signed_txn)
    words = list(struct.unpack("<25Q", ir.to_bytes()))
    witness = {t: [list(it) for it in items] for t, items in ir.witness}
    witness[3] = [list(s) for s in ir.keccak_inputs]
    return Case("decoded_entry", words[1] & ~0xFF, tuple(words[11:18]), witness, OK, None), words


# ---- the entry points that need a device, called as the C ABI has them (null pointers included) ----
def build_state(pg):
    b = pg.ProverStateBuilder()
    for t, name in enumerate(pg.TABLES):
        getattr(b, "set_%s_circuit_size" % name)(range(CFG["table_log_lo"][t], CFG["table_log_hi"][t]))
    b.set(**{k: v for k, v in CFG.items() if not k.startswith("table_")}, n_workers=2, arena_bytes=256 << 20)
    return b.build()


def _call(pg, st, entry, case, words, with_flag):
    """(status, message, bytes or None) of a bp_generate_* entry that takes an IR and a bp_txn_witness"""
    import ctypes as C
    import struct
    L = pg._bind()
    f = getattr(L, entry)
    ir = struct.pack("<25Q", *(words or ir_words(case)))
    w, keep = witness_struct(pg, case)
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    rc = f(st._h, ir, len(ir), C.byref(w) if w is not None else None, *[None] * with_flag, C.byref(out), C.byref(n))
    del keep
    return rc, L.bp_last_error().decode() if rc else "", pg.take_buffer(out, n) if rc == 0 else None


def table_proofs(pg, st, case, words=None):
    return _call(pg, st, "bp_generate_txn_table_proofs", case, words, 1)


def txn_proof(pg, st, case, words=None):
    return _call(pg, st, "bp_generate_txn_proof_witness", case, words, 1)


def preflight_report(pg, st, case, words=None):
    """(status, message, the pg.WitnessReport) of bp_check_txn_witness"""
    import ctypes as C
    import struct
    L = pg._bind()
    ir = struct.pack("<25Q", *(words or ir_words(case)))
    w, keep = witness_struct(pg, case)
    rep = pg.WitnessReport()
    rc = L.bp_check_txn_witness(st._h, ir, len(ir), C.byref(w) if w is not None else None, C.byref(rep))
    del keep
    return rc, L.bp_last_error().decode() if rc else "", rep


def preflight(pg, st, case, words=None):
    """(status, message) of bp_check_txn_witness"""
    return preflight_report(pg, st, case, words)[:2]
