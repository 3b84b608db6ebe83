"""include/bpg.h as Python sees it: the struct mirrors, the prototype of every function and the constants the package uses.
Stated once, here; _lib applies PROTOTYPES to the handles it loads, tests/test_abi_binding.py holds this file to the header."""
import ctypes as C
from ctypes import POINTER as P

vp, cp, i, sz, dbl = C.c_void_p, C.c_char_p, C.c_int, C.c_size_t, C.c_double
u8, u32, u64, i32, i64 = C.c_uint8, C.c_uint32, C.c_uint64, C.c_int32, C.c_int64
u8p, u32p, u64p, i32p, szp = P(u8), P(u32), P(u64), P(i32), P(sz)
u8pp = P(u8p)

# ---- bp_status, and the #defines the package uses
BP_OK, BP_ERR_ABORTED, BP_ERR_INVALID_INPUT, BP_ERR_RANGE, BP_ERR_DEVICE, BP_ERR_VERIFY, BP_ERR_UNSUPPORTED = 0, -1, -2, -3, -4, -5, -6
STATUS_NAMES = {v: k for k, v in list(globals().items()) if k == "BP_OK" or k.startswith("BP_ERR_")}
BP_SET_SKIP_LINK_CHECK = 1
BP_NUM_TABLES, BP_IR_WORDS, BP_PV_WORDS = 7, 25, 13

# the bp_tune_* knobs bp_debug_tune_state lists, in its order (BPG_KNOBS, csrc/tune.cpp; their defaults: csrc/tune.hpp)
KNOBS = ("quad_threshold", "assume_loaded", "merkle_fused", "merkle_wide", "poseidon_mx", "poseidon_mx_sets",
         "poseidon_grouped", "ntt_mx", "ntt_split", "k5_spread", "host_wait", "host_poseidon", "rec_batch",
         "witness_threads", "side_lanes")


def _u32s(*names):
    return [(n, u32) for n in names]


# ---- the structs, in the header's order.  Device pointers are c_void_p: callers hold them as integers.
class AirFamily(C.Structure):
    """bp_air_family: a run of constraints of one kind and degree."""
    _fields_ = _u32s("first_index", "count", "kind", "degree")


class AirDesc(C.Structure):
    """bp_air_desc"""
    _fields_ = ([("air_id", u32), ("name", C.c_char * 24)]
                + _u32s("fixed_n_cols", "n_const_max", "degree", "n_cols", "n_aux", "n_air_constraints", "n_ctl_constraints",
                        "n_units", "n_families")
                + [("families", AirFamily * 24)])


class AirViolation(C.Structure):
    """bp_air_violation: one constraint a row of a trace breaks (bp_air_check_trace)."""
    _fields_ = _u32s("row", "constraint", "family", "kind") + [("value", u64)]


class PlonkLayout(C.Structure):
    """bp_plonk_layout"""
    _fields_ = _u32s("pi_len", "n_paths", "path_depth", "path_pi0", "leaf_len")


class StarkCfg(C.Structure):
    """bp_stark_cfg"""
    _fields_ = _u32s("log_n", "n_cols", "n_const", "deg_pow", "rate_bits", "cap_height", "num_queries", "pow_bits", "arity_bits",
                     "final_poly_bits")


class SetTable(C.Structure):
    """bp_set_table: a member of a table set."""
    _fields_ = [("air_id", u32), ("cfg", StarkCfg), ("d_trace", vp), ("stride", u64), ("d_consts", vp), ("pub", u64p)]


class SetPort(C.Structure):
    """bp_set_port: port `port` of table `table` of a set."""
    _fields_ = _u32s("table", "port")


class SetLink(C.Structure):
    """bp_set_link: the looking ports' tuples are the looked port's."""
    _fields_ = [("n_looking", u32), ("looking", SetPort * 8), ("looked", SetPort)]


class SetTableReport(C.Structure):
    """bp_set_table_report: a member's own constraints (bp_check_table_set)."""
    _fields_ = [("n_violated_rows", u64), ("n_viol", u32), ("reserved", u32), ("viol", AirViolation * 8)]


class SetLinkReport(C.Structure):
    """bp_set_link_report: the balance of one link (bp_check_table_set)."""
    _fields_ = [("holds", u32), ("is_log", u32), ("n_looking", u64), ("n_looked", u64), ("n_unbalanced", u64),
                ("first_looking_end", i32), ("bad_filter_end", i32), ("first_looking_row", i64), ("first_looked_row", i64),
                ("bad_filter_row", i64), ("bad_filter_value", u64)]


class SetReport(C.Structure):
    """bp_set_report"""
    _fields_ = [("table", SetTableReport * 8), ("link", SetLinkReport * 16)]


class BpConfig(C.Structure):
    """bp_config"""
    _fields_ = ([("table_log_lo", u32 * BP_NUM_TABLES), ("table_log_hi", u32 * BP_NUM_TABLES)]
                + _u32s("stark_rate_bits", "stark_cap_height", "stark_num_queries", "stark_pow_bits", "arity_bits",
                        "final_poly_bits", "rec_log_n", "rec_n_cols", "rec_n_const", "rec_rate_bits", "rec_num_queries",
                        "rec_pow_bits", "shrink_depth", "rec_air_id")
                + [("device", i32), ("n_workers", u32), ("arena_bytes", u64)])


class TxnWitness(C.Structure):
    """bp_txn_witness: per table with an AIR of its own, the items (pointer, count) and whether they are given"""
    _fields_ = [(n, t) for names in (("keccak_inputs", "n_perms", "has_keccak"), ("logic_ops", "n_logic_ops", "has_logic"),
                                     ("memory_log", "n_memory_ops", "has_memory"),
                                     ("arithmetic_ops", "n_arithmetic_ops", "has_arithmetic"),
                                     ("byte_sequences", "n_byte_sequences", "has_byte_packing"),
                                     ("sponge_rows", "n_sponge_rows", "has_keccak_sponge"))
                for n, t in zip(names, (vp, sz, i))]


class WitnessTable(C.Structure):
    """bp_witness_table"""
    _fields_ = [("checked", u32), ("given", u32), ("n_violated_rows", u64), ("n_viol", u32), ("viol", AirViolation * 8)]


class WitnessLookup(C.Structure):
    """bp_witness_lookup"""
    _fields_ = [("checked", u32), ("holds", u32), ("n_looking", u64), ("n_looked", u64), ("first_looking_row", i64),
                ("first_looked_row", i64)]


class WitnessReport(C.Structure):
    """bp_witness_report"""
    _fields_ = [("table", WitnessTable * 7), ("lookup", WitnessLookup * 3)]


class TxnPlanTable(C.Structure):
    """bp_txn_plan_table"""
    _fields_ = _u32s("air_id", "n_cols", "log_n", "given", "item_words") + [("capacity", u64)]


class TxnPlanLookup(C.Structure):
    """bp_txn_plan_lookup"""
    _fields_ = _u32s("active", "looking_table", "looking_air", "looked_table", "looked_air")


class TxnPlan(C.Structure):
    """bp_txn_plan"""
    _fields_ = [("table", TxnPlanTable * 7), ("lookup", TxnPlanLookup * 3), ("logic_covered", u32), ("sponge_row_limit", u32)]


class GiOptions(C.Structure):
    """bp_gi_options"""
    _fields_ = [("block_number", u64), ("table_log_n", u32 * BP_NUM_TABLES), ("table_width", u32 * BP_NUM_TABLES), ("flags", u32)]


class GiChain(C.Structure):
    """bp_gi_chain: txn number, gas and state root where an entry starts"""
    _fields_ = [("txn_number", u64), ("gas_used", u64), ("state_root", u64 * 4)]


class ShardOptions(C.Structure):
    """bp_shard_options"""
    _fields_ = _u32s("n_threads", "tree_shape")


ShardLeafFn = C.CFUNCTYPE(i, vp, u32, u8pp, szp)                       # bp_shard_leaf_fn
ShardAggFn = C.CFUNCTYPE(i, vp, u8p, sz, i, u8p, sz, i, u8pp, szp)     # bp_shard_agg_fn

# ---- the functions, in the header's order: name -> (restype, argtypes).  Host bytes go in as c_char_p, device buffers
# and opaque handles as c_void_p, the one-byte abort flags (a c_uint8 or a c_bool by reference) as c_void_p too.
_cfg, _conf, _wit, _opt, _gi = P(StarkCfg), P(BpConfig), P(TxnWitness), P(ShardOptions), P(GiOptions)
_trace = (i, [vp, u64, u32, vp, vp])
_check = [u32, _cfg, vp, u64, vp, u64p, u32, u64p, u32p, P(AirViolation), u32, u32p]
_knob, _ir_flag, _buf = (None, [i]), (i, [u64p, i]), [u8pp, szp]
PROTOTYPES = {
    "bp_last_error": (cp, []),
    "bp_version": (cp, []),
    "bp_device_count": (i, []),
    "bp_use_blocking_sync": (i, [i]),
    "bp_host_wait_mode": (i, [i]),
    "bp_ntt_batch": (i, [vp, u32, u32, u64, i, vp]),
    "bp_intt_batch": (i, [vp, u64, vp, u64, u32, u32, vp]),
    "bp_lde_batch": (i, [vp, u64, vp, u64, vp, u64, u32, u32, u32, i, vp]),
    "bp_debug_copy_u64": (i, [vp, vp, u64, vp]),
    "bp_debug_field_ops": (i, [vp, vp, vp, u64, vp]),
    "bp_debug_lazy_forms": (i, [vp, vp, vp, u64, vp]),
    "bp_debug_plonk_hash_fold": (i, [u64p, vp, vp]),
    "bp_debug_plonk_hash_fold_host": (i, [u64p, u64p]),
    "bp_debug_mul_pow2": (i, [vp, vp, u64, vp]),
    "bp_tune_quad_threshold": (None, [u64]),
    "bp_tune_merkle_fused": _knob,
    "bp_tune_merkle_wide": _knob,
    "bp_tune_poseidon_mx": _knob,
    "bp_tune_poseidon_mx_sets": _knob,
    "bp_tune_poseidon_grouped": _knob,
    "bp_tune_assume_loaded": _knob,
    "bp_tune_rec_batch": _knob,
    "bp_tune_side_lanes": _knob,
    "bp_tune_rec_riders": _knob,
    "bp_tune_txn_group": _knob,
    "bp_tune_rec_group": _knob,
    "bp_debug_rec_batch_histogram": (i, [u64p, u32, i]),
    "bp_tune_witness_threads": _knob,
    "bp_tune_host_wait": _knob,
    "bp_tune_host_poseidon": _knob,
    "bp_debug_poseidon_host": (i, [vp, sz]),
    "bp_tune_k5_spread": _knob,
    "bp_debug_poseidon_group_ops": (u32, [u32]),
    "bp_debug_poseidon_group_tables": (i, [u32, u32, u8p, i32p, i32p, i32p]),
    "bp_tune_ntt_split": _knob,
    "bp_tune_ntt_mx": _knob,
    "bp_tune_reset": (None, []),
    "bp_debug_tune_state": (i, [cp, sz]),
    "bp_debug_ntt_mx_tables": (i, [i, i, u8p, i32p, u64p, u64p]),
    "bp_debug_poseidon_mx_cin": (i, [u32p]),
    "bp_poseidon_perm_batch": (i, [vp, u64, vp]),
    "bp_merkle_digest_words": (u64, [u32, u32]),
    "bp_merkle_commit": (i, [vp, u64, u32, u32, u32, u32, vp, vp]),
    "bp_air_count": (u32, []),
    "bp_air_describe": (i, [u32, u32, u32, u32, P(AirDesc)]),
    "bp_air_register": (i, [vp, sz, u32p]),
    "bp_air_unregister": (i, [u32]),
    "bp_air_program_digest": (i, [u32, cp]),
    "bp_quotient_scratch_words": (u64, [u32, _cfg]),
    "bp_quotient_eval": (i, [u32, _cfg, vp, vp, vp, u64p, u64p, vp, vp, vp]),
    "bp_air_port_products": (i, [u32, _cfg, vp, u64, vp, u64p, u64p, vp, vp]),
    "bp_range_multiplicities": (i, [vp, u64, u32, u64, vp, u32, vp, u64p, vp]),
    "bp_tune_range_lds_log": _knob,
    "bp_debug_air_aux": (i, [u32, _cfg, vp, u64p, vp, vp]),
    "bp_air_check_trace": (i, _check + [vp]),
    "bp_air_check_trace_host": (i, _check),
    "bp_keccak_trace": _trace,
    "bp_logic_trace": _trace,
    "bp_memory_trace": _trace,
    "bp_arithmetic_trace": _trace,
    "bp_byte_packing_trace": _trace,
    "bp_keccak_sponge_trace": _trace,
    "bp_arithmetic_mul_trace": _trace,
    "bp_arithmetic_div_trace": (i, [vp, u32, vp, vp]),
    "bp_arithmetic_div_layout": (i, [u32p, sz]),
    "bp_arithmetic_mod_trace": (i, [vp, u32, vp, vp]),
    "bp_arithmetic_mod_layout": (i, [u32p, sz]),
    "bp_arithmetic_shift_trace": (i, [vp, u32, vp, vp]),
    "bp_arithmetic_shift_layout": (i, [u32p, sz]),
    "bp_arithmetic_sdiv_trace": (i, [vp, u32, vp, vp]),
    "bp_arithmetic_sdiv_layout": (i, [u32p, sz]),
    "bp_arithmetic_exp_trace": (i, [vp, u32, vp, u32, vp, vp]),
    "bp_arithmetic_exp_layout": (i, [u32p, sz]),
    "bp_plonk_constants": (i, [u64, u32, P(PlonkLayout), vp, vp]),
    "bp_plonk_trace": (i, [vp, u64, u64p, P(PlonkLayout), u64p, u32, vp, vp]),
    "bp_fri_fold": (i, [vp, u32, u32, u32, u64, u64p, vp, vp]),
    "bp_openings": (i, [vp, u64, u32, u32, u64p, u64p, vp, vp, vp]),
    "bp_pow_grind": (i, [u64p, u32, u32, u64p, vp]),
    "bp_stark_prove_synthetic": (i, [_cfg, u64, u64, i] + _buf),
    "bp_stark_prove_air": (i, [u32, _cfg, u64, u64, i] + _buf),
    "bp_stark_prove_trace": (i, [u32, _cfg, vp, u64, vp, u64p, i] + _buf),
    "bp_stark_verify_air": (i, [u32, _cfg, u64p, cp, sz]),
    "bp_stark_public_inputs": (None, [u64, u64p]),
    "bp_stark_public_input_list": (None, [u64, u64p]),
    "bp_stark_verify_air_pub": (i, [u32, _cfg, u64p, u64p, cp, sz]),
    "bp_stark_prove_table_set": (i, [P(SetTable), u32, P(SetLink), u32, u32, i] + _buf),
    "bp_stark_verify_table_set": (i, [P(SetTable), u32, P(u64p), P(SetLink), u32, cp, sz]),
    "bp_check_table_set": (i, [P(SetTable), u32, P(SetLink), u32, i, P(SetReport)]),
    "bp_release_cached_memory": (None, []),
    "bp_free_buffer": (None, [u8p]),
    "bp_config_default": (None, [_conf]),
    "bp_state_build": (i, [_conf, P(vp)]),
    "bp_state_free": (None, [vp]),
    "bp_state_device_bytes": (u64, [vp]),
    "bp_state_warnings": (cp, [vp]),
    "bp_state_config": (i, [vp, _conf]),
    "bp_generate_txn_proof": (i, [vp, cp, sz, i32p] + _buf),
    "bp_generate_txn_proof_keccak": (i, [vp, cp, sz, u64p, sz, vp] + _buf),
    "bp_generate_txn_proof_witness": (i, [vp, cp, sz, _wit, vp] + _buf),
    "bp_generate_txn_table_proofs": (i, [vp, cp, sz, _wit, vp] + _buf),
    "bp_generate_txn_table_proofs_group": (i, [vp, cp, sz, u32, vp, vp] + _buf),
    "bp_verify_txn_table_proofs": (i, [_conf, cp, sz]),
    "bp_verify_txn_table_proofs_for": (i, [_conf, cp, sz, cp, sz]),
    "bp_check_txn_witness": (i, [vp, cp, sz, _wit, P(WitnessReport)]),
    "bp_check_txn_witness_keccak": (i, [vp, cp, sz, u64p, sz, P(WitnessReport)]),
    "bp_debug_txn_plan": (i, [_conf, vp, sz, _wit, P(TxnPlan)]),
    "bp_generate_txn_proof_u8": (i, [vp, cp, sz, vp] + _buf),
    "bp_generate_agg_proof": (i, [vp, cp, sz, i, cp, sz, i] + _buf),
    "bp_generate_block_proof": (i, [vp, cp, sz, cp, sz] + _buf + [u64p]),
    "bp_verifier_state_from_prover": (i, [vp, P(vp)]),
    "bp_verifier_state_build": (i, [_conf, P(vp)]),
    "bp_verifier_state_from_caps": (i, [_conf, u64p, P(vp)]),
    "bp_verifier_state_free": (None, [vp]),
    "bp_verify_block_proof": (i, [vp, cp, sz]),
    "bp_verify_proof": (i, [vp, cp, sz]),
    "bp_ir_encode": (i, [u64, u64, u64, u64, u64p, u64, u32p, u32p, u64p]),
    "bp_ir_encode_dummy": (i, [u64, u64, u64, u64p, u64, u32p, u32p, u64p]),
    "bp_ir_set_keccak_air": _ir_flag,
    "bp_ir_set_logic_air": _ir_flag,
    "bp_ir_set_memory_air": _ir_flag,
    "bp_ir_set_arithmetic_air": _ir_flag,
    "bp_ir_set_arithmetic_mul_air": _ir_flag,
    "bp_ir_set_byte_packing_air": _ir_flag,
    "bp_ir_set_keccak_sponge_air": _ir_flag,
    "bp_proof_public_values": (i, [cp, sz, u64p, P(i)]),
    "bp_compact_decode": (i, [cp, sz, u8p, cp, u32p, u32p, u32p, u32p]),
    "bp_compact_decode_full": (i, [cp, sz] + _buf),
    "bp_compact_instructions": (i, [cp, sz] + _buf),
    "bp_keccak256": (None, [cp, sz, cp]),
    "bp_keccak256_permutation_inputs": (i, [cp, sz, cp, u64p, sz, szp]),
    "bp_keccak256_sponge_rows": (i, [cp, sz, cp, u64p, sz, szp]),
    "bp_decode_block_trace": (i, [cp, sz] + _buf),
    "bp_gi_count": (i, [cp, sz, u32p]),
    "bp_gi_chain_start": (i, [cp, sz, P(GiChain)]),
    "bp_gi_entry_ir": (i, [cp, sz, u32, _gi, P(GiChain), u64p]),
    "bp_generate_txn_proof_gi": (i, [vp, cp, sz, u32, _gi, P(GiChain), vp] + _buf),
    "bp_aggregation_plan": (u32, [u32, u32, u32p]),
    "bp_run_shard": (i, [u32, _opt, ShardLeafFn, ShardAggFn, vp, vp] + _buf + _buf),
    "bp_prove_shard": (i, [vp, cp, sz, u32, _opt, vp] + _buf + _buf),
    "bp_aggregate_proofs": (i, [vp, P(cp), szp, u32, _opt] + _buf),
    "bp_prove_shard_gi": (i, [vp, cp, sz, u32, u32, _gi, _opt, vp] + _buf + _buf),
    "bp_state_root_after": (i, [u64p, u64, u64, u64p]),
    "bp_profile_enable": (None, [i]),
    "bp_profile_reset": (None, []),
    "bp_profile_read": (i, [i, u64p, P(dbl), P(dbl)]),
}
