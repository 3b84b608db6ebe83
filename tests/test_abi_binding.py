"""proof_protocol_decoder_amd/_abi.py -- the Python statement of include/bpg.h -- held to the header: every prototype by a
rule written out below, every struct mirror by the sizes and offsets a C compiler gives the header's own structs, the
constants by their values.  Host only: the header is parsed here, a small C program is compiled with gcc."""
import ctypes as C
import os
import re
import subprocess

import pytest

from proof_protocol_decoder_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")

SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
           "double": C.c_double}
POINTEES = dict(SCALARS, uint8_t=C.c_uint8, char=C.c_char, int64_t=C.c_int64)   # what a pointer may point to
CALLBACKS = {"bp_shard_leaf_fn": _abi.ShardLeafFn, "bp_shard_agg_fn": _abi.ShardAggFn}
OPAQUE = ("bp_state", "bp_verifier_state")


def header():
    text = open(os.path.join(INCLUDE, "bpg.h")).read()
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def header_prototypes():
    """[(name, return type, [parameter, ...])] in the header's order"""
    found = re.findall(r"^([\w \*]+?)\s*\b(bp_\w+)\s*\(([^()]*)\)\s*;", header(), flags=re.M)
    return [(name, " ".join(ret.split()), [] if params.strip() == "void" else [" ".join(p.split()) for p in params.split(",")])
            for ret, name, params in found]


def header_callbacks():
    """{typedef name: (return type, [parameter, ...])} of the function-pointer typedefs"""
    found = re.findall(r"typedef\s+(\w+)\s*\(\*(bp_\w+)\)\s*\(([^()]*)\)\s*;", header())
    return {name: (ret, [" ".join(p.split()) for p in params.split(",")]) for ret, name, params in found}


def header_structs():
    """{struct name: [member name, ...]} of every typedef struct with a body"""
    out = {}
    for name, body in re.findall(r"typedef\s+struct\s+(bp_\w+)\s*\{(.*?)\}\s*\1\s*;", header(), flags=re.S):
        out[name] = [re.search(r"(\w+)\s*(?:\[\w+\])?\s*$", part).group(1)
                     for decl in body.split(";") if decl.strip() for part in decl.split(",")]
    return out


def mirror_of(struct_name):
    """bp_air_family -> _abi.AirFamily; bp_config alone keeps its prefix (BpConfig)"""
    camel = "".join(w.capitalize() for w in struct_name[3:].split("_"))
    return getattr(_abi, {"Config": "BpConfig"}.get(camel, camel), None)


def split_param(text):
    """'const uint64_t ctl[4]' -> ('uint64_t', 1): the base type and how many levels of pointer (an array is one)"""
    text = re.sub(r"\b(const|volatile|struct)\b", " ", text)
    m = re.match(r"^\s*(\w+)\s*((?:\*\s*)*)(\w+)?\s*(\[\w*\])?\s*$", text)
    assert m, "cannot parse the parameter %r" % text
    return m.group(1), m.group(2).count("*") + (1 if m.group(4) else 0)


def is_pointer_type(t):
    return isinstance(t, type) and issubclass(t, C._Pointer)


def pointer_ok(t, base):
    """The compatibility rule for one level of pointer to `base`."""
    if t is C.c_void_p:
        return True                                   # every pointer may be stated as void*
    if base == "void" or base in OPAQUE:
        return False                                  # ... and these only so
    if base in POINTEES:
        return t is C.POINTER(POINTEES[base]) or (base in ("uint8_t", "char") and t is C.c_char_p)
    mirror = mirror_of(base)
    return mirror is not None and t is C.POINTER(mirror)


def param_ok(t, text):
    """The compatibility rule for a parameter: scalars by exactly their ctypes type, callbacks by the module's
    CFUNCTYPE, pointers and arrays by pointer_ok, a pointer to a pointer by POINTER(a permitted pointer) or void*."""
    base, depth = split_param(text)
    if depth == 0:
        return t is (CALLBACKS[base] if base in CALLBACKS else SCALARS.get(base))
    if depth == 1:
        return pointer_ok(t, base)
    return depth == 2 and (t is C.c_void_p or (is_pointer_type(t) and pointer_ok(t._type_, base)))


def return_ok(t, text):
    if text == "void":
        return t is None
    if text == "const char*":
        return t is C.c_char_p
    return t is SCALARS.get(text)


def signature_problems(name, restype, argtypes, ret, params):
    if len(argtypes) != len(params):
        return ["%s: %d parameters in the header, %d in the table" % (name, len(params), len(argtypes))]
    bad = [] if return_ok(restype, ret) else ["%s: returns %r, the table says %r" % (name, ret, restype)]
    return bad + ["%s: parameter %d is %r, the table says %r" % (name, k, p, t)
                  for k, (t, p) in enumerate(zip(argtypes, params)) if not param_ok(t, p)]


def test_the_table_states_every_prototype_of_the_header_once_and_compatibly():
    protos = header_prototypes()
    names = [name for name, _, _ in protos]
    assert len(names) == len(set(names)) and len(names) >= 134, "a name is declared twice, or the pattern lost some"
    assert list(_abi.PROTOTYPES) == names, "names and order: in the header only %s, in the table only %s" % (
        sorted(set(names) - set(_abi.PROTOTYPES)), sorted(set(_abi.PROTOTYPES) - set(names)))
    problems = []
    for name, ret, params in protos:
        restype, argtypes = _abi.PROTOTYPES[name]
        problems += signature_problems(name, restype, argtypes, ret, params)
    callbacks = header_callbacks()
    assert set(callbacks) == set(CALLBACKS)
    for name, (ret, params) in callbacks.items():
        problems += signature_problems(name, CALLBACKS[name]._restype_, CALLBACKS[name]._argtypes_, ret, params)
    assert not problems, "\n".join(problems)


def test_the_loaded_library_carries_the_table():
    import proof_protocol_decoder_amd as pkg
    L = pkg.lib()
    assert type(L) is C.CDLL
    for name, (restype, argtypes) in _abi.PROTOTYPES.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    with pytest.raises(TypeError):
        L.bp_merkle_digest_words(3)          # one argument too few never reaches the library


def test_a_prototype_assigned_on_the_public_handle_does_not_reach_the_packages_calls():
    """lib() is what tests, tools and bench.py hold, and they may re-type its functions (with a mirror of their own, as
    tests here did for years); the package calls through _lib.own(), the same library behind other function objects."""
    import proof_protocol_decoder_amd as pkg
    from proof_protocol_decoder_amd import _lib, block_driver
    L = pkg.lib()
    assert L is not _lib.own() and L._handle == _lib.own()._handle
    fn, table = L.bp_aggregation_plan, _abi.PROTOTYPES["bp_aggregation_plan"][1]
    try:
        fn.argtypes = [C.c_uint32, C.c_uint32, C.POINTER(C.c_uint16)]
        with pytest.raises(C.ArgumentError):
            fn(3, 0, (C.c_uint32 * 4)())
        assert block_driver.aggregation_plan(3) == [(0, 1), (3, 2)]
    finally:
        fn.argtypes = table


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    """What gcc makes of the header: {"sizeof <struct>": n, "offsetof <struct> <member>": n, "value <constant>": n}, the
    members asked about being the MIRRORS' -- a name the header does not have fails to compile."""
    status = re.search(r"typedef\s+enum\s*\{(.*?)\}\s*bp_status", header(), flags=re.S).group(1)
    constants = re.findall(r"\b(BP_\w+)\s*=", status) + ["BP_NUM_TABLES", "BP_IR_WORDS", "BP_PV_WORDS", "BP_SET_SKIP_LINK_CHECK"]
    lines = ['#include <stdio.h>', '#include "bpg.h"', "int main(void) {"]
    for struct in header_structs():
        lines.append('  printf("sizeof %s %%zu\\n", sizeof(%s));' % (struct, struct))
        for member, _ in getattr(mirror_of(struct), "_fields_", []):
            lines.append('  printf("offsetof %s %s %%zu\\n", offsetof(%s, %s));' % (struct, member, struct, member))
    lines += ['  printf("value %s %%lld\\n", (long long)%s);' % (c, c) for c in constants]
    lines += ["  return 0;", "}"]
    d = tmp_path_factory.mktemp("abi")
    (d / "layout.c").write_text("\n".join(lines) + "\n")
    cc = subprocess.run(["gcc", "-std=c99", "-I", INCLUDE, "-o", str(d / "layout"), str(d / "layout.c")],
                        capture_output=True, text=True)
    assert cc.returncode == 0, "a mirror names a member its struct does not have:\n" + cc.stderr
    out = subprocess.run([str(d / "layout")], capture_output=True, text=True, check=True).stdout
    return {line.rsplit(" ", 1)[0]: int(line.rsplit(" ", 1)[1]) for line in out.splitlines()}


def test_every_struct_has_a_mirror_of_the_same_layout(compiled):
    structs = header_structs()
    assert len(structs) >= 21 and not set(structs) & set(OPAQUE)
    mirrors = {v for v in vars(_abi).values() if isinstance(v, type) and C.Structure in v.__mro__[1:]}
    assert mirrors == {mirror_of(s) for s in structs}, "one mirror per struct of the header, and nothing else"
    problems = []
    for struct, members in structs.items():
        mirror = mirror_of(struct)
        if [n for n, _ in mirror._fields_] != members:
            problems.append("%s: members %s, the mirror has %s" % (struct, members, [n for n, _ in mirror._fields_]))
        if C.sizeof(mirror) != compiled["sizeof " + struct]:
            problems.append("%s: %d bytes, the mirror has %d" % (struct, compiled["sizeof " + struct], C.sizeof(mirror)))
        for n, _ in mirror._fields_:
            if getattr(mirror, n).offset != compiled["offsetof %s %s" % (struct, n)]:
                problems.append("%s.%s: at byte %d, in the mirror at %d" % (struct, n, compiled["offsetof %s %s" % (struct, n)],
                                                                           getattr(mirror, n).offset))
    assert not problems, "\n".join(problems)


def test_the_constants_are_the_headers(compiled):
    values = {k.split()[1]: v for k, v in compiled.items() if k.startswith("value ")}
    assert len(values) == 11
    for name, value in values.items():
        assert getattr(_abi, name) == value, name
    assert _abi.STATUS_NAMES == {v: k for k, v in values.items() if k == "BP_OK" or k.startswith("BP_ERR_")}
