"""The ctypes view of a C header: `parse(text)` turns the structs and prototypes of include/como_hip.h into ctypes Structures and
(restype, argtypes) pairs, so that the binding in _lib.py is derived from the one declaration the library is compiled against.

Mapping: int / long / float / double -> c_int / c_long / c_float / c_double, como_stream_t -> c_void_p; a return type of void ->
None, void* -> c_void_p; every pointer parameter or field -> c_void_p (an integer device address), except a pointer to one of the
header's structs -> POINTER(Structure) and a pointer whose parameter name ends in `_host` (the header's rule for host memory):
const int* / long* / float* -> POINTER(c_int / c_long / c_float), `T* const*` -> POINTER(c_void_p).
Anything else -- another type word, an array, a bit-field, a function pointer, a struct by value or nested, a conditional other than
the include guard and the __cplusplus blocks -- raises RuntimeError naming the declaration: nothing is guessed, nothing skipped.
"""
import ctypes
import re

SCALARS = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float, "double": ctypes.c_double,
           "como_stream_t": ctypes.c_void_p}
POINTEES = {"void", "int", "long", "float", "double", "uint8_t", "unsigned"}     # what a device pointer may point at
HOST = {t: ctypes.POINTER(SCALARS[t]) for t in ("int", "long", "float")}
RETURNS = {**SCALARS, "void": None, "void*": ctypes.c_void_p}
_STRUCT = re.compile(r"\s*typedef struct (\w+) \{([^{}]*)\} \1;")
_PROTO = re.compile(r"\s*(\w+)\s*(\*?)\s*\b(como_\w+)\s*\((.*)\)\s*", flags=re.S)


def _refuse(decl, why, where=""):
    return RuntimeError(f"como_hip.h: cannot bind `{' '.join(decl.split())}`{where and ' of ' + where} ({why})")


def _declarator(decl, where):
    """`const float* const* K_host` -> ("float", "*const*", "K_host")"""
    toks = re.findall(r"\w+|\S", decl)
    if not all(re.fullmatch(r"\w+|\*", t) for t in toks):
        raise _refuse(decl, "array, bit-field, function pointer or nested declaration", where)
    if len(toks) < 2 or not re.fullmatch(r"[A-Za-z_]\w*", toks[-1]):
        raise _refuse(decl, "no name", where)
    name, ptr = toks.pop(), ""
    if toks[0] == "const":
        toks.pop(0)
    while len(toks) > 1 and toks[-1] in ("*", "const"):
        ptr = toks.pop() + ptr
    return " ".join(toks), ptr, name


def _ctype(decl, structs, where, param):
    base, ptr, name = _declarator(decl, where)
    if not ptr and base in SCALARS:
        return name, SCALARS[base]
    if ptr not in ("*", "*const*") or base not in POINTEES and base not in structs:
        raise _refuse(decl, f"unknown type `{base}{ptr}`", where)
    if param and ptr == "*" and base in structs:
        return name, ctypes.POINTER(structs[base])
    if param and name.endswith("_host"):
        if ptr == "*" and base not in HOST:
            raise _refuse(decl, f"no host array type for `{base}`", where)
        return name, HOST[base] if ptr == "*" else ctypes.POINTER(ctypes.c_void_p)
    return name, ctypes.c_void_p


def _fields(body, structs, where):
    fields = []
    for decl in filter(str.strip, body.split(";")):
        first, *more = decl.split(",")
        name, ctype = _ctype(first, structs, where, param=False)
        if more and "*" in first or not all(re.fullmatch(r"\s*[A-Za-z_]\w*\s*", m) for m in more):
            raise _refuse(decl, "one pointer or plain names per declaration", where)
        fields += [(n.strip(), ctype) for n in [name, *more]]
    return fields


def parse(text):
    """-> ({struct name: ctypes.Structure subclass}, {function name: (restype, [argtypes])}), both in declaration order"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"^#ifdef __cplusplus\n(extern \"C\" \{|\})\n#endif$", "", text, flags=re.M)
    guard = re.search(r"^#ifndef (\w+)\n#define \1$", text, flags=re.M)
    allowed = {"#endif", *(guard.group(0).split("\n") if guard else ())}
    for line in re.findall(r"^[ \t]*#.*$", text, flags=re.M):
        if line.strip() not in allowed and not re.fullmatch(r"#include <\w+\.h>", line.strip()):
            raise _refuse(line, "only the include guard and the __cplusplus blocks may be conditional")
    text = re.sub(r"^[ \t]*#.*$", "", text, flags=re.M)
    structs, functions, pos = {}, {}, 0
    while text[pos:].strip():
        m = _STRUCT.match(text, pos)
        if m and m.group(1) not in structs:
            structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {"_fields_": _fields(m.group(2), structs, m.group(1))})
            pos = m.end()
            continue
        end = text.find(";", pos)
        stmt, pos = (text[pos:], len(text)) if end < 0 else (text[pos:end], end + 1)
        if end >= 0 and re.fullmatch(r"\s*typedef void\s*\* como_stream_t\s*", stmt):
            continue
        m = _PROTO.fullmatch(stmt)
        if end < 0 or not m or m.group(1) + m.group(2) not in RETURNS or m.group(3) in functions:
            raise _refuse(stmt, "not a struct typedef or a `RET como_name(ARGS);` prototype with a known return type")
        args = [] if m.group(4).strip() == "void" else m.group(4).split(",")
        functions[m.group(3)] = (RETURNS[m.group(1) + m.group(2)], [_ctype(arg, structs, m.group(3), param=True)[1] for arg in args])
    return structs, functions
