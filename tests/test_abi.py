"""The C-ABI shared library: builds in-tree, loads without a GPU and exports every symbol include/como_hip.h declares."""
import ctypes
import os
import re

from tests.conftest import ROOT


def declared_symbols():
    hdr = open(os.path.join(ROOT, "include", "como_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    return sorted(set(re.findall(r"\b(como_[a-z0-9_]+)\s*\(", hdr)))


def test_library_exports_every_declared_symbol():
    from como_amd import _lib, build
    build.build()
    L = _lib.lib()
    names = declared_symbols()
    assert len(names) >= 15
    for n in names:
        assert hasattr(L, n), f"{n} declared in include/como_hip.h but not exported"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in como_amd/_lib.py"
    assert set(_lib.SIGNATURES) == set(names)
    assert L.como_abi_version() == 2
    assert L.como_select_workspace_bytes() == 6 * 2048 * 4
    assert L.como_ba_partials_elems(14, 55, 64) == 14 * 55 * 3936


def test_ba_args_struct_matches_header_field_order():
    from como_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "como_hip.h")).read()
    body = hdr[hdr.index("typedef struct como_ba_args {"):hdr.index("} como_ba_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split("{", 1)[1].split(";"):
        decl = decl.strip()
        if not decl:
            continue
        names = decl.replace("*", " ").split()
        for nm in " ".join(names[1:]).split(","):
            nm = nm.strip().split()[-1] if nm.strip() else ""
            if nm and nm not in ("const", "void", "int", "long", "double", "uint8_t"):
                fields.append(nm)
    assert fields == [f[0] for f in _lib.BAArgs._fields_]


def test_win_args_struct_matches_header_field_order():
    from como_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "como_hip.h")).read()
    body = hdr[hdr.index("typedef struct como_win_args {"):hdr.index("} como_win_args;")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S).split("{", 1)[1]
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        toks = decl.replace("*", " ").replace(",", " ").split()
        fields += [t for t in toks if t not in ("const", "void", "int", "long", "double", "uint8_t")]
    assert fields == [f[0] for f in _lib.WinArgs._fields_]


def test_product_never_imports_the_oracle():
    bad = []
    for base, _, files in os.walk(os.path.join(ROOT, "como_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(base, f)).read()
                if re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M):
                    bad.append(os.path.join(base, f))
    assert not bad, f"product code imports the oracle: {bad}"


def test_missing_library_fails_loudly(monkeypatch):
    from como_amd import _lib
    import pytest
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/libcomo_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.lib()


# ---- the binding is derived from the header (como_amd/_abi.py): layouts against the C compiler, signatures against literals ----

def header_text():
    with open(os.path.join(ROOT, "include", "como_hip.h")) as f:
        return f.read()


def host_c_compiler():
    """cc, else the clang of the ROCm tree whose hipcc como_amd/build.py uses"""
    import shutil
    hipcc = os.path.realpath(os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"))
    clang = os.path.join(os.path.dirname(os.path.dirname(hipcc)), "lib", "llvm", "bin", "clang")
    cc = shutil.which("cc") or (clang if os.path.exists(clang) else None)
    assert cc, f"no host C compiler: neither cc on PATH nor {clang}"
    return cc


def test_struct_mirrors_match_the_compiled_header(tmp_path):
    """sizeof and every offsetof of the three argument structs, as the C compiler lays them out, equal the derived ctypes
    Structures' (como_dr_fuse included); compiling with -std=c99 -Wall -Werror also proves the public header is valid C."""
    import subprocess
    from como_amd import _lib
    mirrors = {"como_ba_args": _lib.BAArgs, "como_dr_fuse": _lib.DRFuse, "como_win_args": _lib.WinArgs}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "como_hip.h"', 'int main(void) {']
    for cname, S in mirrors.items():
        lines.append(f'  printf("{cname} sizeof %zu\\n", sizeof({cname}));')
        lines += [f'  printf("{cname} {f} %zu\\n", offsetof({cname}, {f}));' for f, _ in S._fields_]
    lines += ['  return 0;', '}', '']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.run([host_c_compiler(), "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                   check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {tuple(l.split()[:2]): int(l.split()[2]) for l in out.splitlines()}
    want = {}
    for cname, S in mirrors.items():
        want[(cname, "sizeof")] = ctypes.sizeof(S)
        want.update({(cname, f): getattr(S, f).offset for f, _ in S._fields_})
    assert len(want) == 138 + 3
    assert got == want


def test_signatures_pinned_by_hand():
    """One function of every kind, written out as the hand-kept table had it (the *_host arrays of como_track_reference_pyr_f32 typed)."""
    from ctypes import POINTER, c_double, c_float, c_int, c_long, c_void_p
    from como_amd import _lib
    P = c_void_p
    want = {
        "como_abi_version": (c_int, []),
        "como_track_level_workspace_create": (c_void_p, []),
        "como_track_level_workspace_destroy": (None, [P]),
        "como_track_partials_bytes": (c_long, []),
        "como_track_level_f32": (c_int, [P, P, P, P, P, P, c_int, c_int, c_long, P, P, c_int, c_float, c_float, c_float, P, c_int, P, P]),
        "como_kf_distill_prep_f64": (c_int, [P, c_long, P, c_long, c_double, P, c_double, P, c_int, P, P, P, P, P]),
        "como_cross_covariance_f16": (c_int, [P, P, P, P, c_float, P, c_int, c_int, c_int, POINTER(c_long), P]),
        "como_ba_linearize_f64": (c_int, [POINTER(_lib.BAArgs), P]),
        "como_dense_ref_fused_f32": (c_int, [P, c_long, P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, P, c_int,
                                             POINTER(_lib.DRFuse), P]),
        "como_win_logz_ahead": (c_int, [POINTER(_lib.WinArgs), P, c_long, P, P, c_long, P]),
        "como_track_reference_pyr_f32": (c_int, [P, c_int, c_int, P, c_int, c_int, POINTER(c_int), POINTER(P), POINTER(P), POINTER(P),
                                                 POINTER(P), POINTER(P), POINTER(P), c_float, c_float, P]),
    }
    assert len(_lib.SIGNATURES) == 145
    for name, sig in want.items():
        assert _lib.SIGNATURES[name] == sig, name


def test_parser_refuses_what_it_cannot_type(monkeypatch, tmp_path):
    """Every construct the mapping has no rule for raises RuntimeError naming the declaration; nothing defaults to int or is skipped.
    _lib passes a missing or refused header on as a RuntimeError naming its path."""
    import pytest
    from como_amd import _abi, _lib
    ok = "typedef struct s { int a, b; const void* p; } s;\nint como_f(const s* args_host, long n, float* x);\n"
    structs, functions = _abi.parse(ok)
    assert structs["s"]._fields_ == [("a", ctypes.c_int), ("b", ctypes.c_int), ("p", ctypes.c_void_p)]
    assert functions == {"como_f": (ctypes.c_int, [ctypes.POINTER(structs["s"]), ctypes.c_long, ctypes.c_void_p])}
    cases = [
        ("int como_f(unsigned n);", "unsigned n"),                                      # unknown type words
        ("int como_f(long long n);", "long long n"),
        ("int como_f(short n);", "short n"),
        ("int como_f(char c);", "char c"),
        ("int como_f(size_t n);", "size_t n"),
        ("int como_f(const char* name);", "const char* name"),
        ("typedef struct s { short a; } s;", "short a"),
        ("size_t como_f(void);", "size_t como_f"),
        ("int como_f(const double* x_host);", "const double* x_host"),                  # a host array without a rule
        ("int como_f(void (*cb)(int), int n);", "void (*cb)(int)"),                     # function pointer
        ("int como_f(int n[4]);", "int n[4]"),                                          # array declarators
        ("typedef struct s { float v[3]; } s;", "float v[3]"),
        ("typedef struct s { int a : 3; } s;", "int a : 3"),                            # bit-field
        ("typedef struct s { struct { int x; } in; } s;", "struct { int x"),            # nested / anonymous struct
        ("typedef struct { int x; } s;", "typedef struct { int x"),
        ("typedef struct s { int x; } s;\nint como_f(s by_value);", "s by_value"),      # struct by value
        ("typedef struct s { int x; } s;\ntypedef struct t { s inner; } t;", "s inner"),
        ("typedef struct s { int *a, b; } s;", "int *a, b"),
        ("#ifdef COMO_EXTRA\nint como_f(void);\n#endif", "#ifdef COMO_EXTRA"),          # conditionals
        ("#if 1\nint como_f(void);\n#endif", "#if 1"),
        ("#define COMO_N 4\nint como_f(void);", "#define COMO_N 4"),
        ("int como_f(void);\nint x = 3;", "int x = 3"),                                 # statements that are no prototype
        ("int other_f(void);", "int other_f(void)"),
        ("int como_f(int);", "`int` of como_f"),
        ("int como_f(void);\nint como_f(void);", "int como_f(void)"),
        ("int como_f(void)", "int como_f(void)"),
    ]
    for text, offending in cases:
        with pytest.raises(RuntimeError) as e:
            _abi.parse(text)
        assert offending in str(e.value), (text, str(e.value))
    bad = tmp_path / "como_hip.h"
    for path, why in ((str(tmp_path / "absent.h"), "No such file"), (str(bad), "short n")):
        bad.write_text("int como_f(short n);\n")
        monkeypatch.setattr(_lib, "HEADER_PATH", path)
        with pytest.raises(RuntimeError, match=re.escape(path)) as e:
            _lib._load_abi()
        assert why in str(e.value)


def test_host_pointers_are_typed():
    """A parameter named *_host is a typed POINTER (ctypes then rejects a device address or a wrong array at the call); every other
    pointer parameter is a bare c_void_p.  The parameters are read here with a crude parse of their own, not with _abi."""
    import pytest
    from ctypes import POINTER, byref, c_float, c_int, c_long, c_void_p
    from como_amd import _lib
    hdr = re.sub(r"/\*.*?\*/", "", header_text(), flags=re.S)
    hdr = re.sub(r"typedef struct \w+ \{.*?\} \w+;", "", hdr, flags=re.S)
    nfun = nhost = nptr = 0
    for name, params in re.findall(r"\b(como_\w+)\s*\(([^()]*)\)\s*;", hdr):
        params = [] if params.strip() == "void" else [p.strip() for p in params.split(",")]
        argtypes = _lib.SIGNATURES[name][1]
        assert len(argtypes) == len(params), name
        nfun += 1
        for p, t in zip(params, argtypes):
            if p.endswith("_host"):
                nhost += 1
                assert "*" in p and issubclass(t, ctypes._Pointer), (name, p, t)
            elif "*" in p:
                nptr += 1
                assert t is c_void_p, (name, p, t)
    assert nfun == len(_lib.SIGNATURES) and nptr > 0
    assert nhost == 5 + 3 + 2 + 11                              # argument structs, strides, the fuse struct, host arrays
    assert _lib.SIGNATURES["como_nn_normalize_f32"][1][4:6] == [POINTER(c_float)] * 2
    assert _lib.SIGNATURES["como_track_frame_pyramid3_f32"][1][6:8] == [POINTER(c_void_p), POINTER(c_long)]
    for argtype, good in ((POINTER(c_int), (c_int * 8)()), (POINTER(c_long), (c_long * 3)()), (POINTER(c_void_p), (c_void_p * 4)()),
                          (POINTER(c_float), (c_float * 3)()), (POINTER(_lib.BAArgs), byref(_lib.BAArgs()))):
        argtype.from_param(good)
    for argtype in (POINTER(c_int), POINTER(c_long), POINTER(c_float)):
        with pytest.raises(TypeError):
            argtype.from_param(0x7F0000001000)                  # an integer address, as data_ptr() gives
        with pytest.raises(TypeError):
            argtype.from_param((ctypes.c_double * 3)())
