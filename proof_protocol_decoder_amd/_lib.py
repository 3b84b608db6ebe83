"""ctypes loader for libbpg.so (C ABI: include/bpg.h, stated for Python in _abi.py).  Fails loudly when the library is
missing."""
import ctypes as C
import os
import threading

from . import _abi
from ._abi import (BP_ERR_VERIFY, BP_OK, BP_SET_SKIP_LINK_CHECK, KNOBS, STATUS_NAMES, AirDesc, AirFamily,  # noqa: F401
                   AirViolation, SetLink, SetLinkReport, SetPort, SetReport, SetTable, SetTableReport, StarkCfg)

_HERE = os.path.dirname(os.path.abspath(__file__))
# BPG_LIBBPG: another build of the same library (a host-sanitizer build, csrc/Makefile with OUT= / CXXFLAGS=)
_PATH = os.environ.get("BPG_LIBBPG") or os.path.join(_HERE, "lib", "libbpg.so")


class BpgError(RuntimeError):
    """Mirror of the reference's ProofGenError(String) (proof_gen.rs:22-36) with the status code."""

    def __init__(self, code, message):
        super().__init__("%s: %s" % (STATUS_NAMES.get(code, str(code)), message))
        self.code = code
        self.message = message


def take_buffer(ptr, length):
    """Copy a library-allocated buffer into bytes and release it with bp_free_buffer."""
    try:
        return C.string_at(ptr, length.value)
    finally:
        own().bp_free_buffer(ptr)


def call_for_buffer(fn, *args):
    """fn(*args, &out, &out_len), checked: the buffer the library returns through its last two parameters, as bytes."""
    out, n = C.POINTER(C.c_uint8)(), C.c_size_t()
    check(fn(*args, C.byref(out), C.byref(n)))
    return take_buffer(out, n)


def lib_path():
    return _PATH


_handles = {}
_lock = threading.Lock()


def _handle(key):
    """A plain ctypes.CDLL on the library with every prototype of _abi.PROTOTYPES applied -- once, under the lock, before
    any caller sees it.  A name the loaded build does not export (BPG_LIBBPG: an older build) is skipped; calling it
    raises AttributeError."""
    L = _handles.get(key)
    if L is not None:
        return L
    with _lock:
        if key not in _handles:
            if not os.path.exists(_PATH):
                raise ImportError(
                    "libbpg.so not built at %s -- run `python -c 'import __graft_entry__ as g; g.build()'` "
                    "(hipcc --offload-arch=gfx950). There is no CPU fallback for the hot path." % _PATH)
            L = C.CDLL(_PATH)
            for name, (restype, argtypes) in _abi.PROTOTYPES.items():
                fn = getattr(L, name, None)
                if fn is not None:
                    fn.restype, fn.argtypes = restype, argtypes
            _handles[key] = L
    return _handles[key]


def lib():
    """The handle for callers outside the package: tests, tools, bench.py.  Its prototypes stay assignable."""
    return _handle("lib")


def own():
    """The handle the package itself calls through: the same library (one dlopen), function objects of its own, so a
    prototype somebody assigns on lib() -- another mirror of the same struct, say -- never changes how the package calls."""
    return _handle("own")


def check(rc):
    if rc != BP_OK:
        raise BpgError(rc, own().bp_last_error().decode("utf-8", "replace"))
