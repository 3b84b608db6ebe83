"""Shared by tests/test_air_check.py and tests/test_gpu_air_check.py: the oracle's statement of which rows of a trace
violate an AIR (oracle/*_air.c, orc_*_constraints_base, called per row with the selectors of the trace domain), and
its per-constraint values recovered from the fold."""
import ctypes as C

import numpy as np

from builtin_airs import AIRS, P


class OrcConsumer(C.Structure):
    """orc_consumer (oracle/oracle.h): acc_j = acc_j * alpha_j + c in list order; z_last / l_first / l_last multiply
    the transition / first-row / last-row constraints"""
    _fields_ = [(n, C.c_uint64 * 2) for n in ("alpha", "acc")] + [(n, C.c_uint64) for n in ("z_last", "l_first", "l_last")]


_ORC = {}


def oracle_fn(oracle, air_id):
    """a handle of its own on liboracle.so (argument types set here do not touch pyoracle's)"""
    if air_id not in _ORC:
        L = C.CDLL(oracle._LIB_PATH)
        f = getattr(L, AIRS[air_id].constraints)
        f.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(OrcConsumer)]
        f.restype = None
        _ORC[air_id] = f
    return _ORC[air_id]


def omega(log_n):
    return pow(7, (P - 1) >> log_n, P)


def selectors(i, log_n):
    """(z_last, l_first, l_last) of the trace domain at row i"""
    n, w = 1 << log_n, omega(log_n)
    return (pow(w, i, P) - pow(w, n - 1, P)) % P, int(i == 0), int(i == n - 1)


def oracle_fold(oracle, air_id, trace, i, alphas):
    """the oracle's two folds of row i (loc = row i, nxt = row i + 1 mod n)"""
    log_n = trace.shape[1].bit_length() - 1
    loc = np.ascontiguousarray(trace[:, i])
    nxt = np.ascontiguousarray(trace[:, (i + 1) % trace.shape[1]])
    k = OrcConsumer()
    k.alpha[0], k.alpha[1] = int(alphas[0]), int(alphas[1])
    k.z_last, k.l_first, k.l_last = selectors(i, log_n)
    oracle_fn(oracle, air_id)(loc.ctypes.data, nxt.ctypes.data, C.byref(k))
    return int(k.acc[0]), int(k.acc[1])


def oracle_violated_rows(oracle, air_id, trace, seed=1):
    rng = np.random.default_rng(seed)
    alphas = [int(x) % P for x in rng.integers(2, 1 << 62, size=2)]
    return {i for i in range(trace.shape[1]) if any(oracle_fold(oracle, air_id, trace, i, alphas))}


def _intt(vals):
    """inverse NTT over Goldilocks (natural order in, natural order out)"""
    n = len(vals)
    a = list(vals)
    j = 0
    for i in range(1, n):  # bit reversal
        bit = n >> 1
        while j & bit:
            j ^= bit
            bit >>= 1
        j |= bit
        if i < j:
            a[i], a[j] = a[j], a[i]
    length = 2
    while length <= n:
        w = pow(omega(length.bit_length() - 1), P - 2, P)
        for s in range(0, n, length):
            wk = 1
            for t in range(length // 2):
                u, v = a[s + t], a[s + t + length // 2] * wk % P
                a[s + t], a[s + t + length // 2] = (u + v) % P, (u - v) % P
                wk = wk * w % P
        length <<= 1
    inv_n = pow(n, P - 2, P)
    return [x * inv_n % P for x in a]


def oracle_constraint_values(oracle, air_id, trace, i, n_constraints):
    """c_idx at row i, selector applied, recovered by interpolating the fold sum_idx c_idx alpha^(T-1-idx) over alpha"""
    log_m = max(1, (n_constraints - 1).bit_length())
    m = 1 << log_m
    w = omega(log_m)
    folds = [oracle_fold(oracle, air_id, trace, i, (pow(w, k, P), 1))[0] for k in range(m)]
    coeffs = _intt(folds)
    assert all(c == 0 for c in coeffs[n_constraints:]), "the oracle emitted more than the list"
    return [coeffs[n_constraints - 1 - idx] for idx in range(n_constraints)]
