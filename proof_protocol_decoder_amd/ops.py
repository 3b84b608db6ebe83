"""L0 kernel-shaped operations on torch device buffers (thin wrappers over the C ABI).

torch is used only for device memory and streams (int64 tensors carry the u64 bit patterns).
Layouts are the ones documented in include/bpg.h: column-major matrices, natural-order values,
bit-reversed coefficients, coset-major LDE.
"""
import contextlib
import ctypes as C

import numpy as np
import torch

from ._lib import KNOBS, StarkCfg, call_for_buffer, check, lib, own  # noqa: F401 (lib: for callers of ops.lib)

NTT_FWD_BR2NAT, NTT_INV_NAT2BR, NTT_FWD_NAT, NTT_INV_NAT = 0, 1, 2, 3


def _stream():
    return torch.cuda.current_stream().cuda_stream


_tuned_active = False


@contextlib.contextmanager
def tuned(**knobs):
    """Set the named bp_tune_* knobs (tuned(ntt_mx=0, ntt_split=2) calls bp_tune_ntt_mx(0), bp_tune_ntt_split(2)) for
    the body; on the way out, exception or not, bp_tune_reset() puts EVERY knob back to the library's default.
    So blocks do not nest: an inner one would drop the outer one's knobs on its way out, and is refused."""
    global _tuned_active
    if _tuned_active:
        raise RuntimeError("ops.tuned() inside ops.tuned(): name all the knobs in one call")
    unknown = sorted(set(knobs) - set(KNOBS))
    if unknown:
        raise TypeError("no such knob: %s (there are: %s)" % (", ".join(unknown), ", ".join(KNOBS)))
    L = own()
    _tuned_active = True
    try:
        for name, value in knobs.items():
            getattr(L, "bp_tune_" + name)(value)
        yield
    finally:
        _tuned_active = False
        L.bp_tune_reset()


def tune_state():
    """bp_debug_tune_state: the current value of every knob, "name=value" lines in a fixed order."""
    buf = C.create_string_buffer(1024)
    check(own().bp_debug_tune_state(buf, len(buf)))
    return buf.value.decode()


def _require_cuda(t):
    if not t.is_cuda:
        raise ValueError("bpg ops need device tensors (there is no CPU fallback)")
    if t.dtype != torch.int64 or not t.is_contiguous():
        raise ValueError("bpg ops need contiguous int64 tensors holding u64 bit patterns")


def ntt_batch_(cols, direction):
    """In-place NTT of a [n_cols, n] column-major batch."""
    _require_cuda(cols)
    n_cols, n = cols.shape
    check(own().bp_ntt_batch(cols.data_ptr(), n.bit_length() - 1, n_cols, n, direction, _stream()))
    return cols


def intt_batch(values, out=None):
    """Out-of-place inverse NTT: values [n_cols, n] natural -> coefficients (bit-reversed, scaled by 1/n)."""
    _require_cuda(values)
    n_cols, n = values.shape
    out = torch.empty_like(values) if out is None else out
    check(own().bp_intt_batch(values.data_ptr(), n, out.data_ptr(), n, n.bit_length() - 1, n_cols, _stream()))
    return out


def lde_batch(inp, rate_bits, from_coeffs=False):
    """values/coeffs [n_cols, n] -> (coeffs [n_cols, n] bit-reversed, lde [n_cols, n << rate_bits] coset-major)."""
    _require_cuda(inp)
    n_cols, n = inp.shape
    coeffs = torch.empty_like(inp)
    lde = torch.empty((n_cols, n << rate_bits), dtype=torch.int64, device=inp.device)
    check(own().bp_lde_batch(inp.data_ptr(), n, coeffs.data_ptr(), n, lde.data_ptr(), n << rate_bits,
                             n.bit_length() - 1, rate_bits, n_cols, int(from_coeffs), _stream()))
    return coeffs, lde


def poseidon_perm_batch_(states):
    _require_cuda(states)
    check(own().bp_poseidon_perm_batch(states.data_ptr(), states.numel() // 12, _stream()))
    return states


def field_ops(a, b):
    """bp_debug_field_ops: [15, n] planes of canonical results for operand vectors a, b (any u64 patterns)."""
    _require_cuda(a)
    _require_cuda(b)
    n = a.numel()
    out = torch.empty((15, n), dtype=torch.int64, device=a.device)
    check(own().bp_debug_field_ops(a.data_ptr(), b.data_ptr(), out.data_ptr(), n, _stream()))
    return out


def lazy_forms(a, b):
    """bp_debug_lazy_forms: [12, n] planes of the words the lazily reduced forms return, as they return them (any u64
    representative): a*b by gl::mul, the four slots of gl::mul_n<4>, the three of gl::mul_n<3>, a + canon(b),
    a - canon(b), 7*a, a^7; a, b: any u64 patterns."""
    _require_cuda(a)
    _require_cuda(b)
    n = a.numel()
    out = torch.empty((12, n), dtype=torch.int64, device=a.device)
    check(own().bp_debug_lazy_forms(a.data_ptr(), b.data_ptr(), out.data_ptr(), n, _stream()))
    return out


PLONK_HASH_FOLD_WORDS = 2 * 118 + 2   # plonk::HASH_FOLD_WORDS of csrc/air.hpp (tests/test_plonk_hash_fold_model.py compares them)


def plonk_hash_fold(alphas, device="cuda"):
    """bp_debug_plonk_hash_fold: the 238 words with which AIR 8's quotient weighs the S-box outputs of its Poseidon gate
    for the challenge pair `alphas`, as the quotient's launch leaves them on the device: [118][2] = {-C_0, -C_1}, then
    K_0, K_1 (tools/plonk_hash_fold_model.py: pair_table)."""
    out = torch.empty(PLONK_HASH_FOLD_WORDS, dtype=torch.int64, device=device)
    check(own().bp_debug_plonk_hash_fold((C.c_uint64 * 2)(*[int(x) for x in alphas]), out.data_ptr(), _stream()))
    return out


def plonk_hash_fold_host(alphas):
    """bp_debug_plonk_hash_fold_host: the same words by the recurrences on the host (no device is touched)"""
    out = np.zeros(PLONK_HASH_FOLD_WORDS, dtype=np.uint64)
    check(own().bp_debug_plonk_hash_fold_host((C.c_uint64 * 2)(*[int(x) for x in alphas]),
                                              out.ctypes.data_as(C.POINTER(C.c_uint64))))
    return out


def mul_pow2(a):
    """bp_debug_mul_pow2: [21, n] planes, plane 3(k-1) + f = a * 2^(12k) mod p (canonical), k = 1..7, by the groups of
    four (f = 0), of three (f = 1) and the one-element form (f = 2); a: any u64 patterns."""
    _require_cuda(a)
    n = a.numel()
    out = torch.empty((21, n), dtype=torch.int64, device=a.device)
    check(own().bp_debug_mul_pow2(a.data_ptr(), out.data_ptr(), n, _stream()))
    return out


AIR_SYNTHETIC, AIR_KECCAK_F = 0, 1
KECCAK_COLS = 2431
LOGIC_COLS = 524
MEMORY_COLS = 45
ARITHMETIC_COLS = 309
BYTE_PACKING_COLS = 299
KECCAK_SPONGE_COLS = 2414
ARITHMETIC_MUL_COLS = 1217
# the built-in table AIRs by id: (name in bp_<name>_trace, trace width, shape of the caller's inputs at 2^log_n rows)
AIR_TRACES = {1: ("keccak", KECCAK_COLS, lambda log_n: (((1 << log_n) + 23) // 24, 25)),
              2: ("logic", LOGIC_COLS, lambda log_n: (1 << log_n, 9)),
              3: ("memory", MEMORY_COLS, lambda log_n: (1 << log_n, 11)),
              4: ("arithmetic", ARITHMETIC_COLS, lambda log_n: (1 << log_n, 9)),
              5: ("byte_packing", BYTE_PACKING_COLS, lambda log_n: (1 << log_n, 6)),
              6: ("keccak_sponge", KECCAK_SPONGE_COLS, lambda log_n: (1 << log_n, 44)),
              7: ("arithmetic_mul", ARITHMETIC_MUL_COLS, lambda log_n: (1 << log_n, 9))}
AIR_COLS = {air_id: n_cols for air_id, (_, n_cols, _) in AIR_TRACES.items()}


def air_describe(air_id, n_cols=0, n_const=0, deg_pow=1):
    """bp_air_describe: shape and constraint list of a built-in AIR."""
    from ._lib import AirDesc
    d = AirDesc()
    check(own().bp_air_describe(air_id, n_cols, n_const, deg_pow, C.byref(d)))
    return d


def air_register(words):
    """bp_air_register: registers a constraint program (air_program.Builder.assemble(), or any uint64 words of the format in
    include/bpg.h) and returns its air_id, 0x80000000 | 31 bits of the Keccak-256 of its bytes: the same in every process.
    Every entry that takes an air_id takes it.  Registering the same words again returns the same id."""
    words = np.ascontiguousarray(words, dtype=np.uint64)
    air_id = C.c_uint32()
    check(own().bp_air_register(words.ctypes.data, words.size, C.byref(air_id)))
    return air_id.value


def air_unregister(air_id):
    """bp_air_unregister: forgets a registered program (and frees its device images)."""
    check(own().bp_air_unregister(air_id))


def air_program_digest(air_id):
    """bp_air_program_digest: the Keccak-256 of a registered program's bytes."""
    out = C.create_string_buffer(32)
    check(own().bp_air_program_digest(air_id, out))
    return out.raw


def air_trace(air_id, log_n, seed=0, inputs=None, device="cuda"):
    """bp_<name>_trace of the built-in table AIR `air_id` (1..7): the [n_cols, 2^log_n] witness from `inputs` (int64 on the
    device, in the shape AIR_TRACES gives) or drawn from `seed`."""
    name, n_cols, in_shape = AIR_TRACES[air_id]
    out = torch.empty((n_cols, 1 << log_n), dtype=torch.int64, device=device)
    if inputs is not None:
        _require_cuda(inputs)
        assert inputs.shape == in_shape(log_n)
    check(getattr(own(), "bp_%s_trace" % name)(inputs.data_ptr() if inputs is not None else None, seed, log_n, out.data_ptr(),
                                               _stream()))
    return out


def logic_trace(log_n, seed=0, inputs=None, device="cuda"):
    """bp_logic_trace: the AIR-2 witness [524, 2^log_n]; inputs [2^log_n, 9] int64 on the device (operation code, the
    four words of operand 0, of operand 1), or drawn from `seed`."""
    return air_trace(2, log_n, seed, inputs, device)


def memory_trace(log_n, seed=0, inputs=None, device="cuda"):
    """bp_memory_trace: the AIR-3 witness [45, 2^log_n]; inputs [2^log_n, 11] int64 on the device (is_read, address,
    timestamp, eight value limbs; sorted by address then timestamp), or a log drawn from `seed`."""
    return air_trace(3, log_n, seed, inputs, device)


def arithmetic_trace(log_n, seed=0, inputs=None, device="cuda"):
    """bp_arithmetic_trace: the AIR-4 witness [309, 2^log_n]; inputs [2^log_n, 9] int64 on the device (operation code
    0 none / 1 add / 2 sub / 3 lt / 4 gt, the four words of x, of y), or drawn from `seed`."""
    return air_trace(4, log_n, seed, inputs, device)


def byte_packing_trace(log_n, seed=0, inputs=None, device="cuda"):
    """bp_byte_packing_trace: the AIR-5 witness [299, 2^log_n]; inputs [2^log_n, 6] int64 on the device (is_read, len,
    the 32 byte slots as four words), or drawn from `seed`."""
    return air_trace(5, log_n, seed, inputs, device)


def keccak_sponge_trace(log_n, seed=0, inputs=None, device="cuda"):
    """bp_keccak_sponge_trace: the AIR-6 witness [2414, 2^log_n]; inputs [2^log_n, 44] int64 on the device (flags, message
    bytes in the block, the block as absorbed, the state before it: proof_gen.keccak256_sponge_rows), or seeded."""
    return air_trace(6, log_n, seed, inputs, device)


def arithmetic_mul_trace(log_n, seed=0, inputs=None, device="cuda"):
    """bp_arithmetic_mul_trace: the AIR-7 witness [1217, 2^log_n]; inputs [2^log_n, 9] int64 on the device (is_mul, the
    four words of x, of y), or drawn from `seed`."""
    return air_trace(7, log_n, seed, inputs, device)


def _word_table_trace(name, n_words, n_cols, log_n, inputs, device):
    """bp_<name>: the witness [n_cols, 2^log_n] of a shipped table from inputs [2^log_n, n_words] on the device"""
    if inputs is not None:
        _require_cuda(inputs)
        if tuple(inputs.shape) != (1 << log_n, n_words):
            raise ValueError("%s: inputs are [%d, %d]: got %s" % (name, 1 << log_n, n_words, tuple(inputs.shape)))
        device = inputs.device
    out = torch.empty((n_cols, 1 << log_n), dtype=torch.int64, device=device)
    check(getattr(own(), "bp_" + name)(inputs.data_ptr() if inputs is not None else None, log_n, out.data_ptr(), _stream()))
    return out


def arithmetic_div_trace(log_n, inputs, device="cuda"):
    """bp_arithmetic_div_trace: the witness [1650, 2^log_n] of the division table (arithmetic_div.py: a shipped program,
    no built-in air_id); inputs [2^log_n, 9] int64 on the device (op 1 div / 2 mod / else padding | exposed << 8, the four
    words of x, of y: arithmetic_div.pack_inputs).  There is no seeded draw: inputs=None is refused by the library."""
    from .arithmetic_div import N_COLS
    return _word_table_trace("arithmetic_div_trace", 9, N_COLS, log_n, inputs, device)


def arithmetic_mod_trace(log_n, inputs, device="cuda"):
    """bp_arithmetic_mod_trace: the witness [2560, 2^log_n] of the modular table (arithmetic_mod.py: a shipped program,
    no built-in air_id); inputs [2^log_n, 13] int64 on the device (op 1 addmod / 2 mulmod / else padding | exposed << 8,
    the four words of a, of b, of m: arithmetic_mod.pack_inputs).  There is no seeded draw: inputs=None is refused by the
    library."""
    from .arithmetic_mod import N_COLS
    return _word_table_trace("arithmetic_mod_trace", 13, N_COLS, log_n, inputs, device)


def arithmetic_shift_trace(log_n, inputs, device="cuda"):
    """bp_arithmetic_shift_trace: the witness [1143, 2^log_n] of the shift table (arithmetic_shift.py: a shipped program,
    no built-in air_id); inputs [2^log_n, 9] int64 on the device (op 1 shl / 2 shr / 3 sar / else padding | exposed << 8,
    the four words of the shift count s, of the value x: arithmetic_shift.pack_inputs).  There is no seeded draw:
    inputs=None is refused by the library."""
    from .arithmetic_shift import N_COLS
    return _word_table_trace("arithmetic_shift_trace", 9, N_COLS, log_n, inputs, device)


def arithmetic_sdiv_trace(log_n, inputs, device="cuda"):
    """bp_arithmetic_sdiv_trace: the witness [2499, 2^log_n] of the signed table (arithmetic_sdiv.py: a shipped program,
    no built-in air_id); inputs [2^log_n, 9] int64 on the device (op 1 sdiv / 2 smod / else padding | exposed << 8, the
    four words of x, of y, two's complement: arithmetic_sdiv.pack_inputs).  There is no seeded draw: inputs=None is
    refused by the library."""
    from .arithmetic_sdiv import N_COLS
    return _word_table_trace("arithmetic_sdiv_trace", 9, N_COLS, log_n, inputs, device)


def arithmetic_exp_trace(log_n, words, starts):
    """bp_arithmetic_exp_trace: the witness [2003, 2^log_n] of the exponentiation table (arithmetic_exp.py: a shipped
    program, no built-in air_id, one exponent bit per row); words [n_ops, 9] int64 on the device (op 1 exp / else padding |
    exposed << 8, the four words of the base, of the exponent) and starts [n_ops + 1] int32 on the device, the exclusive
    prefix sum of the operations' rows: arithmetic_exp.pack_ops.  No operations (words [0, 9], starts [1]) is an all-padding
    trace."""
    from .arithmetic_exp import N_COLS
    _require_cuda(words)
    if words.dim() != 2 or words.shape[1] != 9:
        raise ValueError("arithmetic_exp_trace: words are [n_ops, 9]: got %s" % (tuple(words.shape),))
    n_ops = words.shape[0]
    if not starts.is_cuda or starts.dtype != torch.int32 or not starts.is_contiguous():
        raise ValueError("arithmetic_exp_trace: starts is a contiguous int32 device tensor holding u32 bit patterns")
    if starts.device != words.device:
        raise ValueError("arithmetic_exp_trace: words are on %s, starts on %s" % (words.device, starts.device))
    if tuple(starts.shape) != (n_ops + 1,):
        raise ValueError("arithmetic_exp_trace: starts is [%d]: got %s" % (n_ops + 1, tuple(starts.shape)))
    out = torch.empty((N_COLS, 1 << log_n), dtype=torch.int64, device=words.device)
    check(own().bp_arithmetic_exp_trace(words.data_ptr() if n_ops else None, n_ops, starts.data_ptr() if n_ops else None, log_n,
                                        out.data_ptr(), _stream()))
    return out


def keccak_trace(log_n, seed=0, inputs=None, device="cuda"):
    """bp_keccak_trace: the AIR-1 witness [2431, 2^log_n]; inputs [n_perm, 25] int64 lanes on the device, or drawn
    from `seed`."""
    return air_trace(1, log_n, seed, inputs, device)


def quotient_eval(cfg, trace_lde, aux_lde, const_lde, ctl, alphas, air_id=AIR_SYNTHETIC):
    """bp_quotient_eval: [2, n << rate_bits] quotient values (coset-major) of AIR `air_id`."""
    _require_cuda(trace_lde)
    _require_cuda(aux_lde)
    if const_lde is not None:
        _require_cuda(const_lde)
    rows = trace_lde.shape[1]
    scratch = torch.empty(int(own().bp_quotient_scratch_words(air_id, C.byref(cfg))), dtype=torch.int64,
                          device=trace_lde.device)
    out = torch.empty((2, rows), dtype=torch.int64, device=trace_lde.device)
    check(own().bp_quotient_eval(air_id, C.byref(cfg), trace_lde.data_ptr(), aux_lde.data_ptr(),
                                 const_lde.data_ptr() if const_lde is not None else None,
                                 (C.c_uint64 * 4)(*[int(x) for x in ctl]), (C.c_uint64 * 2)(*[int(x) for x in alphas]),
                                 scratch.data_ptr(), out.data_ptr(), _stream()))
    return out


class AirCheck:
    """What bp_air_check_trace found: how many rows violate the AIR, the first of them (row order) and the constraints
    those rows break (bp_air_violation: row, constraint index, family index into air_describe's families, kind, value
    before the row selector).  `n_violations` counts all of them; at most `max_viol` are in `violations`."""

    def __init__(self, air_id, n_violated_rows, rows, violations, n_violations):
        self.air_id = air_id
        self.n_violated_rows = n_violated_rows
        self.rows = rows
        self.violations = violations
        self.n_violations = n_violations

    @property
    def ok(self):
        return self.n_violated_rows == 0

    def __repr__(self):
        return "AirCheck(air %d: %d violated rows, first %s)" % (self.air_id, self.n_violated_rows, self.rows[:8])


def _check_cfg(air_id, n_cols, n_const, log_n, deg_pow):
    d = air_describe(air_id, n_cols, n_const, deg_pow)
    if d.fixed_n_cols:
        deg_pow = 3 if d.degree > 3 else 1
    return stark_cfg(log_n, n_cols, n_const=n_const, deg_pow=deg_pow, rate_bits=1 if deg_pow == 1 else 3)


def _check_shapes(n, consts, pub):
    """the trace's height is a power of two, the constants are [n_const, n] (read with column stride n), four public inputs"""
    if n < 1 or n & (n - 1):
        raise ValueError("a trace has 2^log_n rows: got %d" % n)
    if consts is not None and (len(consts.shape) != 2 or consts.shape[1] != n):
        raise ValueError("constants must be [n_const, %d]: got %s" % (n, tuple(consts.shape)))
    if pub is not None and len(pub) != 4:
        raise ValueError("four public inputs: got %d" % len(pub))


def _check_call(fn, air_id, cfg, trace_ptr, stride, consts_ptr, pub, max_rows, max_viol, *stream):
    from ._lib import AirViolation
    n_rows, n_viol = C.c_uint64(), C.c_uint32()
    rows = (C.c_uint32 * max(1, max_rows))()
    viol = (AirViolation * max(1, max_viol))()
    pub_arr = (C.c_uint64 * 4)(*[int(x) for x in pub]) if pub is not None else None
    check(fn(air_id, C.byref(cfg), trace_ptr, stride, consts_ptr, pub_arr, max_rows, C.byref(n_rows), rows, viol, max_viol,
             C.byref(n_viol), *stream))
    got_rows = min(n_rows.value, max_rows)
    return AirCheck(air_id, n_rows.value, [int(rows[i]) for i in range(got_rows)],
                    [viol[i] for i in range(min(n_viol.value, max_viol))], n_viol.value)


def check_air_trace(air_id, trace, consts=None, pub=None, max_rows=16, max_viol=None, deg_pow=1):
    """bp_air_check_trace: which rows of `trace` ([n_cols, 2^log_n] on the device; a column slice of a wider buffer
    keeps its stride) violate AIR `air_id`'s own constraints, and which constraints the first `max_rows` of them break.
    consts: [n_const, 2^log_n] (AIR 0 with constants, AIR 8); pub: AIR 8's four public inputs; deg_pow: the synthetic
    AIR's.  Nothing is raised for a bad trace: the result says what is wrong (AirCheck)."""
    if not trace.is_cuda or trace.dtype != torch.int64 or trace.stride(1) != 1:
        raise ValueError("check_air_trace needs an int64 device tensor with contiguous columns")
    n_cols, n = trace.shape
    if consts is not None:
        _require_cuda(consts)
    _check_shapes(n, consts, pub)
    cfg = _check_cfg(air_id, n_cols, consts.shape[0] if consts is not None else 0, n.bit_length() - 1, deg_pow)
    return _check_call(own().bp_air_check_trace, air_id, cfg, trace.data_ptr(), trace.stride(0),
                       consts.data_ptr() if consts is not None else None, pub, max_rows,
                       4 * max_rows + 64 if max_viol is None else max_viol, _stream())


def check_air_trace_host(air_id, trace, consts=None, pub=None, max_rows=16, max_viol=None, deg_pow=1):
    """bp_air_check_trace_host: the same on the CPU, for a numpy uint64 trace [n_cols, 2^log_n] (rows may be strided)."""
    trace = np.asarray(trace)
    if trace.dtype != np.uint64 or trace.strides[1] != 8:
        raise ValueError("check_air_trace_host needs a uint64 array with contiguous columns")
    n_cols, n = trace.shape
    if consts is not None:
        consts = np.ascontiguousarray(consts, dtype=np.uint64)
    _check_shapes(n, consts, pub)
    cfg = _check_cfg(air_id, n_cols, consts.shape[0] if consts is not None else 0, n.bit_length() - 1, deg_pow)
    return _check_call(own().bp_air_check_trace_host, air_id, cfg, trace.ctypes.data, trace.strides[0] // 8,
                       consts.ctypes.data if consts is not None else None, pub, max_rows,
                       4 * max_rows + 64 if max_viol is None else max_viol)


def fri_fold(values, log_nl, rate_bits, shift, beta, arity_bits=4):
    """bp_fri_fold: values [n_l << rate_bits, 2] (coset-major ext elements) -> next layer [(n_l >> 4) << rate_bits, 2]."""
    _require_cuda(values)
    out = torch.empty(((1 << (log_nl - arity_bits)) << rate_bits, 2), dtype=torch.int64, device=values.device)
    check(own().bp_fri_fold(values.data_ptr(), log_nl, rate_bits, arity_bits, int(shift),
                            (C.c_uint64 * 2)(int(beta[0]), int(beta[1])), out.data_ptr(), _stream()))
    return out


def openings(coeffs, z0, z1=None):
    """bp_openings: coeffs [n_cols, n] bit-reversed -> [n_cols, 4] = (p(z0), p(z1)) as extension pairs."""
    _require_cuda(coeffs)
    n_cols, n = coeffs.shape
    pw = torch.empty(4 * n, dtype=torch.int64, device=coeffs.device)
    out = torch.zeros((n_cols, 4), dtype=torch.int64, device=coeffs.device)
    a0 = (C.c_uint64 * 2)(int(z0[0]), int(z0[1]))
    a1 = (C.c_uint64 * 2)(int(z1[0]), int(z1[1])) if z1 is not None else None
    check(own().bp_openings(coeffs.data_ptr(), n, n.bit_length() - 1, n_cols, a0, a1, pw.data_ptr(), out.data_ptr(),
                            _stream()))
    return out


def pow_grind(state, pos, bits):
    """bp_pow_grind: smallest nonce for the 12-word sponge `state` (host ints) with `bits` leading zeros."""
    nonce = C.c_uint64()
    check(own().bp_pow_grind((C.c_uint64 * 12)(*[int(x) for x in state]), pos, bits, C.byref(nonce), _stream()))
    return nonce.value


def merkle_commit(lde, log_n, rate_bits, cap_height):
    """Returns the level-order digest buffer [words/4, 4]; the last 2^cap_height rows are the cap."""
    _require_cuda(lde)
    n_cols, rows = lde.shape
    assert rows == 1 << (log_n + rate_bits)
    words = own().bp_merkle_digest_words(log_n + rate_bits, cap_height)
    dig = torch.empty((words // 4, 4), dtype=torch.int64, device=lde.device)
    check(own().bp_merkle_commit(lde.data_ptr(), rows, n_cols, log_n, rate_bits, cap_height, dig.data_ptr(),
                                 _stream()))
    return dig


def stark_cfg(log_n, n_cols, n_const=0, deg_pow=1, rate_bits=1, cap_height=4, num_queries=84, pow_bits=16,
              arity_bits=4, final_poly_bits=5):
    return StarkCfg(log_n, n_cols, n_const, deg_pow, rate_bits, cap_height, num_queries, pow_bits, arity_bits,
                    final_poly_bits)


def _words(proof_bytes):
    return np.frombuffer(proof_bytes, dtype=np.uint64).copy()


def stark_prove_air(air_id, cfg, seed, const_seed=0, device=0):
    """One table proof on AIR `air_id`, witness generated on the device.  Returns proof words (u64)."""
    return _words(call_for_buffer(own().bp_stark_prove_air, air_id, C.byref(cfg), seed, const_seed, device))


def stark_prove_trace(air_id, cfg, trace, consts=None, pub=None, device=None):
    """bp_stark_prove_trace: the table proof of stark_prove_air from the caller's trace ([n_cols, 2^log_n] int64 on the
    device, canonical words; a column slice of a wider buffer keeps its stride), for a built-in or a registered air_id.
    consts: [n_const, 2^log_n]; pub: four public inputs (AIR 8, programs that read some).  Returns proof words (u64)."""
    if not trace.is_cuda or trace.dtype != torch.int64 or trace.stride(1) != 1:
        raise ValueError("stark_prove_trace needs an int64 device tensor with contiguous columns")
    if consts is not None:
        _require_cuda(consts)
    _check_shapes(trace.shape[1], consts, pub)
    if trace.shape[0] != cfg.n_cols or trace.shape[1] != 1 << cfg.log_n:
        raise ValueError("the trace is %s, the configuration says [%d, %d]" % (tuple(trace.shape), cfg.n_cols, 1 << cfg.log_n))
    torch.cuda.synchronize(trace.device)  # the library proves on a stream of its own
    pub_arr = (C.c_uint64 * 4)(*[int(x) for x in pub]) if pub is not None else None
    dev = trace.device.index if device is None else device
    return _words(call_for_buffer(own().bp_stark_prove_trace, air_id, C.byref(cfg), trace.data_ptr(), trace.stride(0),
                                  consts.data_ptr() if consts is not None else None, pub_arr, dev or 0))


def air_port_products(air_id, trace, ctl, consts=None, pub=None):
    """bp_air_port_products: the running products [2 * n_ports, 2^log_n] of a registered program's lookup ports over
    `trace` ([n_cols, 2^log_n] int64 on the device; a column slice of a wider buffer keeps its stride): port l's z_0 at
    row 2l, z_1 at 2l + 1; a log port's running sums in the same rows.  ctl = beta0, gamma0, beta1, gamma1."""
    if not trace.is_cuda or trace.dtype != torch.int64 or trace.stride(1) != 1:
        raise ValueError("air_port_products needs an int64 device tensor with contiguous columns")
    n_cols, n = trace.shape
    if consts is not None:
        _require_cuda(consts)
    _check_shapes(n, consts, pub)
    d = air_describe(air_id)
    cfg = _check_cfg(air_id, n_cols, consts.shape[0] if consts is not None else 0, n.bit_length() - 1, 1)
    out = torch.empty((d.n_aux, n), dtype=torch.int64, device=trace.device)
    pub_arr = (C.c_uint64 * 4)(*[int(x) for x in pub]) if pub is not None else None
    check(own().bp_air_port_products(air_id, C.byref(cfg), trace.data_ptr(), trace.stride(0),
                                     consts.data_ptr() if consts is not None else None, pub_arr,
                                     (C.c_uint64 * 4)(*[int(x) for x in ctl]), out.data_ptr(), _stream()))
    return out


def range_multiplicities(values, log_range, filter=None, out=None):
    """bp_range_multiplicities: how often each value of [0, 2^log_range) occurs in `values` ([n_cols, n_rows] int64 on the
    device; a column slice of a wider buffer keeps its stride) on the rows where `filter` ([n_rows] of 0 / 1; None = all) is
    set.  The counts are ADDED to `out` ([2^log_range] int64; None = a fresh zeroed one), which is returned.  A kept value
    outside the range raises BpgError(BP_ERR_RANGE); its .first_bad is the smallest col * n_rows + row holding one."""
    from ._lib import BpgError
    if not values.is_cuda or values.dtype != torch.int64 or values.dim() != 2 or values.stride(1) != 1:
        raise ValueError("range_multiplicities needs a 2-d int64 device tensor with contiguous columns")
    n_cols, n_rows = values.shape
    if filter is not None:
        _require_cuda(filter)
        if filter.shape != (n_rows,):
            raise ValueError("the filter has one word per row")
    if out is None:
        out = torch.zeros(1 << log_range, dtype=torch.int64, device=values.device)
    _require_cuda(out)
    if out.shape != (1 << log_range,):
        raise ValueError("out holds 2^log_range words")
    first_bad = C.c_uint64()
    try:
        check(own().bp_range_multiplicities(values.data_ptr(), values.stride(0), n_cols, n_rows,
                                            filter.data_ptr() if filter is not None else None, log_range, out.data_ptr(),
                                            C.byref(first_bad), _stream()))
    except BpgError as e:
        e.first_bad = first_bad.value
        raise
    return out


def debug_air_aux(air_id, trace, ctl):
    """bp_debug_air_aux (a test entry): the auxiliary columns [n_aux, 2^log_n] the prover commits for a built-in table
    with a lookup side, from a contiguous trace [n_cols, 2^log_n]."""
    _require_cuda(trace)
    n_cols, n = trace.shape
    _check_shapes(n, None, None)
    cfg = _check_cfg(air_id, n_cols, 0, n.bit_length() - 1, 1)
    out = torch.empty((air_describe(air_id).n_aux, n), dtype=torch.int64, device=trace.device)
    check(own().bp_debug_air_aux(air_id, C.byref(cfg), trace.data_ptr(), (C.c_uint64 * 4)(*[int(x) for x in ctl]), out.data_ptr(), _stream()))
    return out


def _set_arguments(tables, links):
    """(SetTable array, SetLink array, what they point to) from tables = dicts / tuples with air_id, cfg and optionally
    trace, consts, pub, and links = (looking ports, looked port), a port = (table, port)."""
    from ._lib import SetLink, SetPort, SetTable
    keep = []
    ta = (SetTable * max(1, len(tables)))()
    for t, m in zip(ta, tables):
        t.air_id, t.cfg = m["air_id"], m["cfg"]
        trace, consts, pub = m.get("trace"), m.get("consts"), m.get("pub")
        if trace is not None:
            if not trace.is_cuda or trace.dtype != torch.int64 or trace.stride(1) != 1:
                raise ValueError("a set's traces are int64 device tensors with contiguous columns")
            t.d_trace, t.stride = trace.data_ptr(), trace.stride(0)
        if consts is not None:
            _require_cuda(consts)
            t.d_consts = consts.data_ptr()
        if pub is not None:
            arr = (C.c_uint64 * 4)(*[int(x) for x in pub])
            keep.append(arr)
            t.pub = C.cast(arr, C.POINTER(C.c_uint64))
    la = (SetLink * max(1, len(links)))()
    for l, (looking, looked) in zip(la, links):
        l.n_looking = len(looking)
        for k, (table, port) in enumerate(looking[:8]):
            l.looking[k] = SetPort(table, port)
        l.looked = SetPort(*looked)
    return ta, la, keep


def stark_prove_table_set(tables, links, skip_link_check=False, device=0):
    """bp_stark_prove_table_set: the traces of `tables` (dicts: air_id, cfg, trace, and consts / pub where the AIR has
    them), linked port to port by `links` = [([(table, port), ...looking], (table, port) looked), ...], proven on one
    transcript.  Returns the "BPGTSET1" container words (u64).  An unbalanced link raises BpgError(BP_ERR_VERIFY) naming
    it, unless skip_link_check."""
    from ._lib import BP_SET_SKIP_LINK_CHECK
    ta, la, keep = _set_arguments(tables, links)
    if torch.cuda.is_available():
        torch.cuda.synchronize()  # the library proves on a stream of its own
    return _words(call_for_buffer(own().bp_stark_prove_table_set, ta, len(tables), la, len(links),
                                  BP_SET_SKIP_LINK_CHECK if skip_link_check else 0, device))


class SetLinkCheck:
    """bp_set_link_report: does the link hold, and if not which rows unbalance it (include/bpg.h states every field)."""
    FIELDS = ("holds", "is_log", "n_looking", "n_looked", "n_unbalanced", "first_looking_end", "first_looking_row",
              "first_looked_row", "bad_filter_end", "bad_filter_row", "bad_filter_value")

    def __init__(self, r):
        for name in self.FIELDS:
            setattr(self, name, bool(getattr(r, name)) if name in ("holds", "is_log") else int(getattr(r, name)))

    def as_dict(self):
        return {name: getattr(self, name) for name in self.FIELDS}

    def __repr__(self):
        return "SetLinkCheck(%s)" % ", ".join("%s=%s" % kv for kv in self.as_dict().items())


class SetCheck:
    """What bp_check_table_set found: `tables` (an AirCheck per member: its own constraints, the first 8 rows and
    violations), `links` (a SetLinkCheck per link), and the library's sentence about the first finding in `message`
    ("" when the set is fine)."""

    def __init__(self, tables, links, message):
        self.tables = tables
        self.links = links
        self.message = message

    @property
    def ok(self):
        return all(t.ok for t in self.tables) and all(l.holds for l in self.links)

    def __repr__(self):
        return "SetCheck(ok)" if self.ok else "SetCheck(%s)" % self.message


def check_table_set(tables, links, device=0):
    """bp_check_table_set: the pre-flight of stark_prove_table_set on the same arguments -- every member's own
    constraints and every link's balance, computed on the device, nothing proven.  Nothing is raised for a set that would
    not prove (BP_ERR_VERIFY is the answer: SetCheck.ok is False and .message names the first finding); every other status
    raises BpgError."""
    from ._lib import BP_ERR_VERIFY, BpgError, SetReport
    ta, la, keep = _set_arguments(tables, links)
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    rep = SetReport()
    rc = own().bp_check_table_set(ta, len(tables), la, len(links), device, C.byref(rep))
    message = ""
    if rc != 0:
        message = own().bp_last_error().decode("utf-8", "replace")
        if rc != BP_ERR_VERIFY:
            raise BpgError(rc, message)
    checks = []
    for t, m in zip(rep.table, tables):
        k = min(t.n_viol, 8)
        viol = [t.viol[i] for i in range(k)]
        rows = sorted({v.row for v in viol})
        checks.append(AirCheck(m["air_id"], t.n_violated_rows, rows, viol, t.n_viol))
    return SetCheck(checks, [SetLinkCheck(rep.link[k]) for k in range(len(links))], message)


def stark_verify_table_set(tables, links, proof, const_caps=None):
    """bp_stark_verify_table_set: the CPU verifier on a set's container.  The statement -- tables (air_id, cfg, pub; no
    traces), links, const_caps (per table the constants cap words or None) -- is the caller's own.  Raises
    BpgError(BP_ERR_VERIFY) on rejection."""
    ta, la, keep = _set_arguments([{k: v for k, v in m.items() if k not in ("trace", "consts")} for m in tables], links)
    caps = None
    if const_caps is not None:
        caps = (C.POINTER(C.c_uint64) * len(tables))()
        for k, cap in enumerate(const_caps):
            if cap is not None:
                cap = np.ascontiguousarray(cap, dtype=np.uint64)
                keep.append(cap)
                caps[k] = cap.ctypes.data_as(C.POINTER(C.c_uint64))
    proof = np.ascontiguousarray(proof, dtype=np.uint64)
    check(own().bp_stark_verify_table_set(ta, len(tables), caps, la, len(links), proof.tobytes(), proof.size * 8))


def stark_verify_air(air_id, cfg, proof, const_cap=None, pub=None):
    """bp_stark_verify_air_pub: the CPU verifier on one table proof (uint64 words); raises BpgError(BP_ERR_VERIFY) on
    rejection.  const_cap: the constants commitment's cap words when the table has constant columns."""
    proof = np.ascontiguousarray(proof, dtype=np.uint64)
    cap = None
    if const_cap is not None:
        const_cap = np.ascontiguousarray(const_cap, dtype=np.uint64)
        cap = const_cap.ctypes.data_as(C.POINTER(C.c_uint64))
    pub_arr = (C.c_uint64 * 4)(*[int(x) for x in pub]) if pub is not None else None
    check(own().bp_stark_verify_air_pub(air_id, C.byref(cfg), cap, pub_arr, proof.tobytes(), proof.size * 8))


def stark_prove_synthetic(cfg, seed, const_seed=0, device=0):
    """One table proof on the synthetic AIR, witness generated on the device.  Returns proof words (u64)."""
    return _words(call_for_buffer(own().bp_stark_prove_synthetic, C.byref(cfg), seed, const_seed, device))
