"""ctypes loader for libbpg.so (C ABI: include/bpg.h).  Fails loudly when the library is missing."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# BPG_LIBBPG: another build of the same library (a host-sanitizer build, csrc/Makefile with OUT= / CXXFLAGS=)
_PATH = os.environ.get("BPG_LIBBPG") or os.path.join(_HERE, "lib", "libbpg.so")

BP_OK = 0
BP_ERR_VERIFY = -5
STATUS_NAMES = {0: "BP_OK", -1: "BP_ERR_ABORTED", -2: "BP_ERR_INVALID_INPUT", -3: "BP_ERR_RANGE",
                -4: "BP_ERR_DEVICE", -5: "BP_ERR_VERIFY", -6: "BP_ERR_UNSUPPORTED"}


class BpgError(RuntimeError):
    """Mirror of the reference's ProofGenError(String) (proof_gen.rs:22-36) with the status code."""

    def __init__(self, code, message):
        super().__init__("%s: %s" % (STATUS_NAMES.get(code, str(code)), message))
        self.code = code
        self.message = message


class StarkCfg(C.Structure):
    """bp_stark_cfg (include/bpg.h)."""
    _fields_ = [(n, C.c_uint32) for n in ("log_n", "n_cols", "n_const", "deg_pow", "rate_bits", "cap_height",
                                           "num_queries", "pow_bits", "arity_bits", "final_poly_bits")]


class AirFamily(C.Structure):
    """bp_air_family: a run of constraints of one kind and degree."""
    _fields_ = [(n, C.c_uint32) for n in ("first_index", "count", "kind", "degree")]


class AirDesc(C.Structure):
    """bp_air_desc (include/bpg.h)."""
    _fields_ = ([("air_id", C.c_uint32), ("name", C.c_char * 24)]
                + [(n, C.c_uint32) for n in ("fixed_n_cols", "n_const_max", "degree", "n_cols", "n_aux",
                                             "n_air_constraints", "n_ctl_constraints", "n_units", "n_families")]
                + [("families", AirFamily * 24)])


class SetTable(C.Structure):
    """bp_set_table: a member of a table set."""
    _fields_ = [("air_id", C.c_uint32), ("cfg", StarkCfg), ("d_trace", C.c_void_p), ("stride", C.c_uint64),
                ("d_consts", C.c_void_p), ("pub", C.POINTER(C.c_uint64))]


class SetPort(C.Structure):
    """bp_set_port: port `port` of table `table` of a set."""
    _fields_ = [("table", C.c_uint32), ("port", C.c_uint32)]


class SetLink(C.Structure):
    """bp_set_link: the looking ports' tuples are the looked port's."""
    _fields_ = [("n_looking", C.c_uint32), ("looking", SetPort * 8), ("looked", SetPort)]


BP_SET_SKIP_LINK_CHECK = 1


class AirViolation(C.Structure):
    """bp_air_violation: one constraint a row of a trace breaks (bp_air_check_trace)."""
    _fields_ = [(n, C.c_uint32) for n in ("row", "constraint", "family", "kind")] + [("value", C.c_uint64)]


class SetTableReport(C.Structure):
    """bp_set_table_report: a member's own constraints (bp_check_table_set)."""
    _fields_ = [("n_violated_rows", C.c_uint64), ("n_viol", C.c_uint32), ("reserved", C.c_uint32), ("viol", AirViolation * 8)]


class SetLinkReport(C.Structure):
    """bp_set_link_report: the balance of one link (bp_check_table_set)."""
    _fields_ = [("holds", C.c_uint32), ("is_log", C.c_uint32), ("n_looking", C.c_uint64), ("n_looked", C.c_uint64),
                ("n_unbalanced", C.c_uint64), ("first_looking_end", C.c_int32), ("bad_filter_end", C.c_int32),
                ("first_looking_row", C.c_int64), ("first_looked_row", C.c_int64), ("bad_filter_row", C.c_int64),
                ("bad_filter_value", C.c_uint64)]


class SetReport(C.Structure):
    """bp_set_report."""
    _fields_ = [("table", SetTableReport * 8), ("link", SetLinkReport * 16)]


def take_buffer(ptr, length):
    """Copy a library-allocated buffer into bytes and release it with bp_free_buffer."""
    try:
        return C.string_at(ptr, length.value)
    finally:
        lib().bp_free_buffer(ptr)


def lib_path():
    return _PATH


# the bp_tune_* knobs (include/bpg.h; their defaults live in csrc/tune.hpp), in bp_debug_tune_state's order
KNOBS = ("quad_threshold", "assume_loaded", "merkle_fused", "merkle_wide", "poseidon_mx", "poseidon_mx_sets",
         "poseidon_grouped", "ntt_mx", "ntt_split", "k5_spread", "host_wait", "host_poseidon", "rec_batch",
         "witness_threads", "side_lanes")

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_PATH):
        raise ImportError(
            "libbpg.so not built at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback for the hot path." % _PATH)
    L = C.CDLL(_PATH)
    vp, u32, u64, i = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int
    L.bp_last_error.restype = C.c_char_p
    L.bp_version.restype = C.c_char_p
    L.bp_device_count.restype = i
    L.bp_ntt_batch.argtypes = [vp, u32, u32, u64, i, vp]
    L.bp_intt_batch.argtypes = [vp, u64, vp, u64, u32, u32, vp]
    L.bp_lde_batch.argtypes = [vp, u64, vp, u64, vp, u64, u32, u32, u32, i, vp]
    L.bp_poseidon_perm_batch.argtypes = [vp, u64, vp]
    L.bp_debug_field_ops.argtypes = [vp, vp, vp, u64, vp]
    L.bp_debug_mul_pow2.argtypes = [vp, vp, u64, vp]
    L.bp_quotient_scratch_words.argtypes = [u32, C.POINTER(StarkCfg)]
    L.bp_quotient_scratch_words.restype = u64
    L.bp_quotient_eval.argtypes = [u32, C.POINTER(StarkCfg), vp, vp, vp, C.POINTER(u64), C.POINTER(u64), vp, vp, vp]
    L.bp_air_count.restype = u32
    L.bp_air_describe.argtypes = [u32, u32, u32, u32, C.POINTER(AirDesc)]
    check_args = [u32, C.POINTER(StarkCfg), vp, u64, vp, C.POINTER(u64), u32, C.POINTER(u64), C.POINTER(u32),
                  C.POINTER(AirViolation), u32, C.POINTER(u32)]
    L.bp_air_check_trace.argtypes = check_args + [vp]
    L.bp_air_check_trace_host.argtypes = check_args
    L.bp_keccak_trace.argtypes = [vp, u64, u32, vp, vp]
    L.bp_logic_trace.argtypes = [vp, u64, u32, vp, vp]
    L.bp_memory_trace.argtypes = [vp, u64, u32, vp, vp]
    L.bp_arithmetic_trace.argtypes = [vp, u64, u32, vp, vp]
    L.bp_byte_packing_trace.argtypes = [vp, u64, u32, vp, vp]
    L.bp_keccak_sponge_trace.argtypes = [vp, u64, u32, vp, vp]
    L.bp_arithmetic_mul_trace.argtypes = [vp, u64, u32, vp, vp]
    L.bp_arithmetic_div_trace.argtypes = [vp, u32, vp, vp]
    L.bp_arithmetic_div_layout.argtypes = [C.POINTER(u32), C.c_size_t]
    L.bp_stark_verify_air.argtypes = [u32, C.POINTER(StarkCfg), C.POINTER(u64), C.c_char_p, C.c_size_t]
    L.bp_stark_prove_air.argtypes = [u32, C.POINTER(StarkCfg), u64, u64, i, C.POINTER(C.POINTER(C.c_uint8)),
                                     C.POINTER(C.c_size_t)]
    L.bp_stark_verify_air_pub.argtypes = [u32, C.POINTER(StarkCfg), C.POINTER(u64), C.POINTER(u64), C.c_char_p, C.c_size_t]
    L.bp_stark_prove_trace.argtypes = [u32, C.POINTER(StarkCfg), vp, u64, vp, C.POINTER(u64), i, C.POINTER(C.POINTER(C.c_uint8)),
                                       C.POINTER(C.c_size_t)]
    L.bp_debug_air_aux.argtypes = [u32, C.POINTER(StarkCfg), vp, C.POINTER(u64), vp, vp]
    L.bp_air_port_products.argtypes = [u32, C.POINTER(StarkCfg), vp, u64, vp, C.POINTER(u64), C.POINTER(u64), vp, vp]
    L.bp_range_multiplicities.argtypes = [vp, u64, u32, u64, vp, u32, vp, C.POINTER(u64), vp]
    L.bp_tune_range_lds_log.argtypes = [i]
    L.bp_tune_range_lds_log.restype = None
    L.bp_stark_prove_table_set.argtypes = [C.POINTER(SetTable), u32, C.POINTER(SetLink), u32, u32, i,
                                           C.POINTER(C.POINTER(C.c_uint8)), C.POINTER(C.c_size_t)]
    L.bp_stark_verify_table_set.argtypes = [C.POINTER(SetTable), u32, C.POINTER(C.POINTER(u64)), C.POINTER(SetLink), u32,
                                            C.c_char_p, C.c_size_t]
    L.bp_check_table_set.argtypes = [C.POINTER(SetTable), u32, C.POINTER(SetLink), u32, i, C.POINTER(SetReport)]
    L.bp_air_register.argtypes = [vp, C.c_size_t, C.POINTER(u32)]
    L.bp_air_unregister.argtypes = [u32]
    L.bp_air_program_digest.argtypes = [u32, C.c_char_p]
    L.bp_fri_fold.argtypes = [vp, u32, u32, u32, u64, C.POINTER(u64), vp, vp]
    L.bp_openings.argtypes = [vp, u64, u32, u32, C.POINTER(u64), C.POINTER(u64), vp, vp, vp]
    L.bp_pow_grind.argtypes = [C.POINTER(u64), u32, u32, C.POINTER(u64), vp]
    L.bp_merkle_digest_words.argtypes = [u32, u32]
    L.bp_merkle_digest_words.restype = u64
    L.bp_merkle_commit.argtypes = [vp, u64, u32, u32, u32, u32, vp, vp]
    L.bp_stark_prove_synthetic.argtypes = [C.POINTER(StarkCfg), u64, u64, i, C.POINTER(C.POINTER(C.c_uint8)),
                                           C.POINTER(C.c_size_t)]
    L.bp_free_buffer.argtypes = [C.POINTER(C.c_uint8)]
    L.bp_free_buffer.restype = None
    for knob in KNOBS:
        fn = getattr(L, "bp_tune_" + knob)
        fn.argtypes = [u64 if knob == "quad_threshold" else i]
        fn.restype = None
    L.bp_tune_reset.argtypes = []
    L.bp_tune_reset.restype = None
    L.bp_debug_tune_state.argtypes = [C.c_char_p, C.c_size_t]
    _lib = L
    return L


def check(rc):
    if rc != BP_OK:
        raise BpgError(rc, lib().bp_last_error().decode("utf-8", "replace"))
