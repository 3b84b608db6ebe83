"""Host-side mirror of the reference's plonky_block_proof_gen API over the C ABI (include/bpg.h).

Same names, argument meaning and error behaviour as the Rust crate:
  ProverStateBuilder / ProverState      plonky_block_proof_gen/src/prover_state.rs:17-100
  generate_txn_proof / agg / block      plonky_block_proof_gen/src/proof_gen.rs:39-110
  GeneratedTxnProof / AggProof / BlockProof / AggregatableProof
                                        plonky_block_proof_gen/src/proof_types.rs:12-87
  VerifierState                         plonky_block_proof_gen/src/verifier_state.rs:19-71
  ProofGenError                         plonky_block_proof_gen/src/proof_gen.rs:16-36
There is no CPU fallback: everything below calls libbpg.so.
"""
import ctypes as C
import struct
from dataclasses import dataclass

from . import _abi
from ._abi import BpConfig, TxnWitness, WitnessLookup, WitnessTable  # noqa: F401
from ._lib import BpgError, call_for_buffer, check, lib, own, take_buffer

NUM_TABLES = _abi.BP_NUM_TABLES
TABLES = ("arithmetic", "byte_packing", "cpu", "keccak", "keccak_sponge", "logic", "memory")
IR_WORDS, PV_WORDS = _abi.BP_IR_WORDS, _abi.BP_PV_WORDS

ProofGenError = BpgError  # Result<T, ProofGenError(String)> -> exception carrying the message
_bind = lib   # every prototype is applied when the library is loaded (_abi.PROTOTYPES); the name stays for its callers
             # outside the package; the calls below go through the package's own handle (_lib.own)

# The AIRs that can prove a table of a transaction instead of the synthetic one (csrc/txn_tables.hpp holds the same rows;
# include/bpg.h lists them above bp_ir_set_*_air): TxnProofGenIR field, table index, AIR id, setter, the bp_txn_witness
# members that carry the table's witness items, u64 words per item.  In the order to_bytes sets the flags.
TXN_TABLE_AIRS = (
    ("keccak_air", 3, 1, "bp_ir_set_keccak_air", ("keccak_inputs", "n_perms", "has_keccak"), 25),
    ("logic_air", 5, 2, "bp_ir_set_logic_air", ("logic_ops", "n_logic_ops", "has_logic"), 9),
    ("memory_air", 6, 3, "bp_ir_set_memory_air", ("memory_log", "n_memory_ops", "has_memory"), 11),
    ("arithmetic_air", 0, 4, "bp_ir_set_arithmetic_air", ("arithmetic_ops", "n_arithmetic_ops", "has_arithmetic"), 9),
    ("byte_packing_air", 1, 5, "bp_ir_set_byte_packing_air", ("byte_sequences", "n_byte_sequences", "has_byte_packing"), 6),
    ("keccak_sponge_air", 4, 6, "bp_ir_set_keccak_sponge_air", ("sponge_rows", "n_sponge_rows", "has_keccak_sponge"), 44),
    ("arithmetic_mul_air", 0, 7, "bp_ir_set_arithmetic_mul_air", ("arithmetic_ops", "n_arithmetic_ops", "has_arithmetic"), 9),
)
# table index -> (pointer, count, has_* member of bp_txn_witness, words per item)
WITNESS_FIELDS = {t: (*members, words) for _, t, _, _, members, words in TXN_TABLE_AIRS}
KECCAK_LANES, SPONGE_ROW_WORDS = WITNESS_FIELDS[3][3], WITNESS_FIELDS[4][3]


@dataclass(frozen=True)
class PublicValues:
    """Subset of plonky2_evm PublicValues carried by the synthetic workload."""
    txn_number_before: int
    txn_number_after: int
    gas_used_before: int
    gas_used_after: int
    state_root_before: tuple
    state_root_after: tuple
    block_number: int

    @classmethod
    def from_words(cls, w):
        return cls(w[0], w[1], w[2], w[3], tuple(w[4:8]), tuple(w[8:12]), w[12])


def state_root_after(root_before, seed, txn_number):
    """bp_state_root_after: the synthetic state transition of one (non-dummy) transaction."""
    out = (C.c_uint64 * 4)()
    check(own().bp_state_root_after((C.c_uint64 * 4)(*root_before), seed, txn_number, out))
    return tuple(out)


def public_values_of(proof_bytes):
    L = own()
    pv = (C.c_uint64 * PV_WORDS)()
    kind = C.c_int()
    check(L.bp_proof_public_values(proof_bytes, len(proof_bytes), pv, C.byref(kind)))
    return PublicValues.from_words(list(pv)), kind.value


@dataclass(frozen=True)
class TxnProofGenIR:
    """Synthetic stand-in for protocol_decoder::types::TxnProofGenIR (= GenerationInputs,
    protocol_decoder/src/types.rs:48): what one txn proof is generated from."""
    block_number: int
    txn_number_before: int
    gas_used_before: int
    gas_used_after: int
    state_root_before: tuple
    seed: int
    table_log_n: tuple
    table_width: tuple
    dummy: bool = False   # a padding entry (decoding.rs:484-520): proven, but txn number / gas / state root stay
    keccak_air: bool = False   # the Keccak table is a real Keccak-f[1600] trace (this and the flags below: TXN_TABLE_AIRS)
    keccak_inputs: tuple = None   # ... attesting THESE permutations ([n][25] lanes) instead of seeded ones; not part of
                                  # the 25-word IR: handed to bp_generate_txn_proof_keccak beside it
    logic_air: bool = False    # the logic table is proven with the logic AIR
    memory_air: bool = False   # the memory table with the memory AIR
    arithmetic_air: bool = False   # the arithmetic table with the arithmetic AIR
    byte_packing_air: bool = False   # the byte-packing table with the byte-packing AIR
    keccak_sponge_air: bool = False  # the Keccak sponge table with the Keccak sponge AIR
    arithmetic_mul_air: bool = False   # the arithmetic table with the multiplication AIR instead (one or the other)
    witness: tuple = None   # ((table index, ((words of an item), ...)), ...): data for tables with an AIR instead of a
                            # seeded witness (bp_generate_txn_proof_witness); like keccak_inputs not part of the 25-word IR

    def to_bytes(self):
        L = own()
        out = (C.c_uint64 * IR_WORDS)()
        root = (C.c_uint64 * 4)(*self.state_root_before)
        logs, widths = (C.c_uint32 * NUM_TABLES)(*self.table_log_n), (C.c_uint32 * NUM_TABLES)(*self.table_width)
        if self.dummy:
            if self.gas_used_after != self.gas_used_before:
                raise ValueError("a dummy entry uses no gas (decoding.rs:503-506)")
            check(L.bp_ir_encode_dummy(self.block_number, self.txn_number_before, self.gas_used_before, root, self.seed,
                                       logs, widths, out))
        else:
            check(L.bp_ir_encode(self.block_number, self.txn_number_before, self.gas_used_before, self.gas_used_after,
                                 root, self.seed, logs, widths, out))
        for field, _, _, setter, _, _ in TXN_TABLE_AIRS:
            if getattr(self, field):
                check(getattr(L, setter)(out, 1))
        return struct.pack("<%dQ" % IR_WORDS, *out)


@dataclass(frozen=True)
class GeneratedTxnProof:
    p_vals: PublicValues
    intern: bytes


@dataclass(frozen=True)
class GeneratedAggProof:
    p_vals: PublicValues
    intern: bytes


@dataclass(frozen=True)
class GeneratedBlockProof:
    b_height: int
    intern: bytes


class AggregatableProof:
    """Sum type Txn | Agg (proof_types.rs:46-87)."""

    def __init__(self, proof):
        if not isinstance(proof, (GeneratedTxnProof, GeneratedAggProof)):
            raise TypeError("AggregatableProof wraps a txn or an agg proof")
        self._p = proof

    def public_values(self):
        return self._p.p_vals

    def is_agg(self):
        return isinstance(self._p, GeneratedAggProof)

    def intern(self):
        return self._p.intern


def _as_aggregatable(p):
    return p if isinstance(p, AggregatableProof) else AggregatableProof(p)


class ProverState:
    """Pre-processed circuits resident in HBM (prover_state.rs:17-20).  Immutable; share freely
    between threads."""

    def __init__(self, handle, cfg):
        self._h, self.cfg = handle, cfg

    @property
    def device_bytes(self):
        return own().bp_state_device_bytes(self._h)

    @property
    def warnings(self):
        """What bp_state_build found about its environment (GPU_MAX_HW_QUEUES below n_workers, the host-wait mode
        the device was left in); "" when there is nothing to say."""
        return own().bp_state_warnings(self._h).decode("utf-8", "replace") if self._h else ""

    def close(self):
        if self._h:
            own().bp_state_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown: module globals may already be gone
            pass


class ProverStateBuilder:
    """Builder with the reference's default ranges (constants.rs:6-18) and
    set_<table>_circuit_size(range) setters (prover_state.rs:55-75)."""

    def __init__(self):
        self.cfg = BpConfig()
        own().bp_config_default(C.byref(self.cfg))

    def _set(self, idx, size):
        self.cfg.table_log_lo[idx], self.cfg.table_log_hi[idx] = size.start, size.stop
        return self

    def set_arithmetic_circuit_size(self, size): return self._set(0, size)
    def set_byte_packing_circuit_size(self, size): return self._set(1, size)
    def set_cpu_circuit_size(self, size): return self._set(2, size)
    def set_keccak_circuit_size(self, size): return self._set(3, size)
    def set_keccak_sponge_circuit_size(self, size): return self._set(4, size)
    def set_logic_circuit_size(self, size): return self._set(5, size)
    def set_memory_circuit_size(self, size): return self._set(6, size)

    def set(self, **kw):
        """Non-reference knobs: device, n_workers, arena_bytes, recursion/STARK shape parameters."""
        for k, v in kw.items():
            if not hasattr(self.cfg, k):
                raise AttributeError(k)
            setattr(self.cfg, k, v)
        return self

    def build(self):
        h = C.c_void_p()
        check(own().bp_state_build(C.byref(self.cfg), C.byref(h)))
        return ProverState(h, self.cfg)

    def build_verifier(self):
        h = C.c_void_p()
        check(own().bp_verifier_state_build(C.byref(self.cfg), C.byref(h)))
        return VerifierState(h)


def _out():
    return C.POINTER(C.c_uint8)(), C.c_size_t()


def keccak256_permutation_inputs(data: bytes):
    """bp_keccak256_permutation_inputs: -> (digest, [n_perms][25] lanes): the states that go into the Keccak-f
    permutations of Keccak-256(data) -- what a Keccak table attesting this hash contains."""
    L = own()
    n = C.c_size_t()
    check(L.bp_keccak256_permutation_inputs(data, len(data), None, None, 0, C.byref(n)))
    k = KECCAK_LANES
    states, digest = (C.c_uint64 * (k * n.value))(), C.create_string_buffer(32)
    check(L.bp_keccak256_permutation_inputs(data, len(data), digest, states, n.value, C.byref(n)))
    return digest.raw, [list(states[k * i:k * i + k]) for i in range(n.value)]


def keccak256_sponge_rows(data: bytes):
    """bp_keccak256_sponge_rows: -> (digest, [n_blocks][44] words): the rows a Keccak sponge table (AIR 6) absorbing
    `data` contains -- flags, message bytes in the block, the block as absorbed, the state before it."""
    L = own()
    n = C.c_size_t()
    check(L.bp_keccak256_sponge_rows(data, len(data), None, None, 0, C.byref(n)))
    k = SPONGE_ROW_WORDS
    rows, digest = (C.c_uint64 * (k * n.value))(), C.create_string_buffer(32)
    check(L.bp_keccak256_sponge_rows(data, len(data), digest, rows, n.value, C.byref(n)))
    return digest.raw, [list(rows[k * i:k * i + k]) for i in range(n.value)]


def generate_txn_proof(p_state, gen_inputs, abort_signal=None, keccak_inputs=None, witness=None):
    """proof_gen.rs:39-56.  abort_signal: optional shared flag (the reference's Option<Arc<AtomicBool>>): a
    ctypes.c_uint8 / c_bool (one byte, what AtomicBool is: bp_generate_txn_proof_u8) or a ctypes.c_int32.
    keccak_inputs: the permutation inputs ([n][25] lanes) of the transaction's Keccak table, for an IR with
    keccak_air=True (bp_generate_txn_proof_keccak); default: gen_inputs.keccak_inputs if it has any.
    witness: {table index: [[words of an item], ...]} for the tables proven with an AIR (TXN_TABLE_AIRS has the words of
    an item; bp_generate_txn_proof_witness); default: gen_inputs.witness."""
    L = own()
    ir = gen_inputs.to_bytes() if isinstance(gen_inputs, TxnProofGenIR) else bytes(gen_inputs)
    flag = C.byref(abort_signal) if abort_signal is not None else None
    if keccak_inputs is None:
        keccak_inputs = getattr(gen_inputs, "keccak_inputs", None)
    if witness is not None or getattr(gen_inputs, "witness", None) is not None:
        if abort_signal is not None and C.sizeof(abort_signal) != 1:
            raise ValueError("bp_generate_txn_proof_witness takes the one-byte abort flag")
        w, keep = _witness_struct(gen_inputs, keccak_inputs, witness)
        intern = call_for_buffer(L.bp_generate_txn_proof_witness, p_state._h, ir, len(ir), C.byref(w), flag)
        del keep
    elif keccak_inputs is not None:
        flat = [int(x) for st in keccak_inputs for x in st]
        arr = (C.c_uint64 * max(len(flat), 1))(*flat)
        if abort_signal is not None and C.sizeof(abort_signal) != 1:
            raise ValueError("bp_generate_txn_proof_keccak takes the one-byte abort flag")
        intern = call_for_buffer(L.bp_generate_txn_proof_keccak, p_state._h, ir, len(ir), arr, len(flat) // KECCAK_LANES, flag)
    elif abort_signal is not None and C.sizeof(abort_signal) == 1:
        intern = call_for_buffer(L.bp_generate_txn_proof_u8, p_state._h, ir, len(ir), flag)
    else:
        intern = call_for_buffer(L.bp_generate_txn_proof, p_state._h, ir, len(ir), flag)
    return GeneratedTxnProof(public_values_of(intern)[0], intern)


def _witness_struct(gen_inputs, keccak_inputs, witness):
    """(TxnWitness or None, the ctypes arrays it points into) from the forms generate_txn_proof accepts."""
    if keccak_inputs is None:
        keccak_inputs = getattr(gen_inputs, "keccak_inputs", None)
    if witness is None and getattr(gen_inputs, "witness", None) is not None:
        witness = dict(gen_inputs.witness)
    if witness is None and keccak_inputs is None:
        return None, []
    witness = dict(witness or {})
    if keccak_inputs is not None and 3 not in witness:
        witness[3] = keccak_inputs
    w, keep = TxnWitness(), []
    for t, items in witness.items():
        ptr_f, n_f, has_f, words = WITNESS_FIELDS[t]
        flat = [int(x) for it in items for x in it]
        if len(flat) % words:
            raise ValueError("witness items of table %d have %d words each" % (t, words))
        a = (C.c_uint64 * max(len(flat), 1))(*flat)
        keep.append(a)
        setattr(w, ptr_f, C.cast(a, C.c_void_p))
        setattr(w, n_f, len(flat) // words)
        setattr(w, has_f, 1)
    return w, keep


def generate_txn_table_proofs(p_state, gen_inputs, keccak_inputs=None, witness=None):
    """What upstream's `prove` yields before the recursion (its AllProof; reached from proof_gen.rs:44-52): the seven
    table proofs of the transaction on their one transcript, with the public values and the lookup challenges, as
    bytes (bp_generate_txn_table_proofs).  Arguments as for generate_txn_proof."""
    ir = gen_inputs.to_bytes() if isinstance(gen_inputs, TxnProofGenIR) else bytes(gen_inputs)
    w, keep = _witness_struct(gen_inputs, keccak_inputs, witness)
    blob = call_for_buffer(own().bp_generate_txn_table_proofs, p_state._h, ir, len(ir), C.byref(w) if w is not None else None, None)
    del keep
    return blob


def generate_txn_table_proofs_group(p_state, gen_inputs_list):
    """bp_generate_txn_table_proofs_group: generate_txn_table_proofs for several transactions at a time, table t of those
    whose shapes agree proved in lock-step on one group of provers.  The blobs are the single call's, byte for byte."""
    L = own()
    irs = [g.to_bytes() if isinstance(g, TxnProofGenIR) else bytes(g) for g in gen_inputs_list]
    n = len(irs)
    if n < 1 or any(len(ir) != len(irs[0]) for ir in irs):
        raise ValueError("one or more IRs of one length")
    structs = [_witness_struct(g, None, None) if isinstance(g, TxnProofGenIR) else (None, []) for g in gen_inputs_list]
    data = (C.c_void_p * n)(*[C.addressof(w) if w is not None else None for w, _ in structs])
    outs, lens = (C.POINTER(C.c_uint8) * n)(), (C.c_size_t * n)()
    raw = b"".join(irs)
    check(L.bp_generate_txn_table_proofs_group(p_state._h, raw, len(irs[0]), n, data, None, outs, lens))
    del structs
    return [take_buffer(outs[i], C.c_size_t(lens[i])) for i in range(n)]


class WitnessReport(_abi.WitnessReport):
    """bp_witness_report with the call's status and message: `ok` when the prover would accept the data"""
    LOOKUPS = ("keccak_sponge -> keccak_f", "byte_packing -> memory", "keccak_sponge -> logic")
    status = 0
    message = ""

    @property
    def ok(self):
        return self.status == 0

    def violations(self, t):
        return list(self.table[t].viol[:self.table[t].n_viol])


def check_txn_witness(p_state, gen_inputs, keccak_inputs=None, witness=None):
    """The witness pre-flight (bp_check_txn_witness): what generate_txn_proof would say about the same inputs, without
    proving -- the tables' AIRs row by row and the three lookups as multisets.  Arguments as for generate_txn_proof.
    Returns a WitnessReport (status 0 = ok, or BP_ERR_VERIFY with the table / row / constraint or the lookup and its
    first unmatched rows in `message`); raises ProofGenError only where the prover would refuse the input."""
    L = own()
    ir = gen_inputs.to_bytes() if isinstance(gen_inputs, TxnProofGenIR) else bytes(gen_inputs)
    rep = WitnessReport()
    if keccak_inputs is None:
        keccak_inputs = getattr(gen_inputs, "keccak_inputs", None)
    if witness is None and getattr(gen_inputs, "witness", None) is None and keccak_inputs is not None:
        flat = [int(x) for st in keccak_inputs for x in st]
        arr = (C.c_uint64 * max(len(flat), 1))(*flat)
        rc = L.bp_check_txn_witness_keccak(p_state._h, ir, len(ir), arr, len(flat) // KECCAK_LANES, C.byref(rep))
    else:
        w, keep = _witness_struct(gen_inputs, keccak_inputs, witness)
        rc = L.bp_check_txn_witness(p_state._h, ir, len(ir), C.byref(w) if w is not None else None, C.byref(rep))
        del keep
    if rc not in (_abi.BP_OK, _abi.BP_ERR_VERIFY):   # a report; anything else is the prover's refusal
        check(rc)
    rep.status = rc
    rep.message = L.bp_last_error().decode("utf-8", "replace") if rc else ""
    return rep


def verify_txn_table_proofs(cfg, table_proofs, gen_inputs=None):
    """upstream's verify_proof(all_stark, all_proof, config) on the CPU: every table proof against the shared transcript
    and the cross-table lookups between the tables proven with their AIRs.  cfg: a BpConfig (ProverState.cfg).
    gen_inputs (a TxnProofGenIR or its bytes): the statement -- which AIR proves each table, the shapes, the public
    values -- is then the verifier's (bp_verify_txn_table_proofs_for); without it the blob's header is taken at its
    word and the caller must check it.  Raises ProofGenError when rejected."""
    L = own()
    b = bytes(table_proofs)
    if gen_inputs is None:
        check(L.bp_verify_txn_table_proofs(C.byref(cfg), b, len(b)))
        return
    ir = gen_inputs.to_bytes() if hasattr(gen_inputs, "to_bytes") else bytes(gen_inputs)
    check(L.bp_verify_txn_table_proofs_for(C.byref(cfg), ir, len(ir), b, len(b)))


def generate_agg_proof(p_state, lhs_child, rhs_child):
    """proof_gen.rs:61-79."""
    lhs, rhs = _as_aggregatable(lhs_child), _as_aggregatable(rhs_child)
    intern = call_for_buffer(own().bp_generate_agg_proof, p_state._h, lhs.intern(), len(lhs.intern()), int(lhs.is_agg()),
                             rhs.intern(), len(rhs.intern()), int(rhs.is_agg()))
    return GeneratedAggProof(public_values_of(intern)[0], intern)


def generate_block_proof(p_state, prev_opt_parent_b_proof, curr_block_agg_proof):
    """proof_gen.rs:85-110."""
    L = own()
    parent = prev_opt_parent_b_proof.intern if prev_opt_parent_b_proof is not None else None
    out, n = _out()
    h = C.c_uint64()
    check(L.bp_generate_block_proof(p_state._h, parent, len(parent) if parent else 0, curr_block_agg_proof.intern,
                                    len(curr_block_agg_proof.intern), C.byref(out), C.byref(n), C.byref(h)))
    return GeneratedBlockProof(h.value, take_buffer(out, n))


class VerifierState:
    """verifier_state.rs:19-23; built from a ProverState (:46-52) or a builder (:34-42)."""

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_prover_state(cls, p_state):
        h = C.c_void_p()
        check(own().bp_verifier_state_from_prover(p_state._h, C.byref(h)))
        return cls(h)

    @classmethod
    def from_caps(cls, cfg, caps_words):
        """Verifier-only deployment (no GPU): cfg is a BpConfig, caps_words the 3 circuit caps."""
        h = C.c_void_p()
        arr = (C.c_uint64 * len(caps_words))(*[int(x) for x in caps_words])
        check(own().bp_verifier_state_from_caps(C.byref(cfg), arr, C.byref(h)))
        return cls(h)

    def verify(self, block_proof):
        """verifier_state.rs:56-71.  Raises ProofGenError when the proof is rejected."""
        b = block_proof.intern if isinstance(block_proof, GeneratedBlockProof) else bytes(block_proof)
        check(own().bp_verify_block_proof(self._h, b, len(b)))

    def verify_any(self, proof):
        b = proof.intern if hasattr(proof, "intern") and not callable(proof.intern) else bytes(proof)
        check(own().bp_verify_proof(self._h, b, len(b)))

    def close(self):
        if self._h:
            own().bp_verifier_state_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass
