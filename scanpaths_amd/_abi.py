"""The C ABI as ctypes, read from include/scanpaths_amd.h: its integer defines, its two descriptor structs and every entry point.

Not a C parser: it knows the few forms the header uses and raises on anything else, naming the declaration, so a new form is added here
on purpose and never guessed.  hip.py parses the header once at import; tests/test_abi.py holds every rule to synthetic text.
"""
import ctypes as C
import os
import re

HEADER_PATH = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "scanpaths_amd.h")
SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "float": C.c_float, "double": C.c_double}


def _scalar(words, where):
    if len(words) != 2 or words[0] not in SCALARS or not words[1].isidentifier():
        raise ValueError(f"{where}: `{' '.join(words)}` is none of {sorted(SCALARS)} or a pointer (scanpaths_amd/_abi.py)")
    return SCALARS[words[0]]


def _fields(body, where):
    """`int a, b;` lists expanded in declaration order; any pointer field is a c_void_p"""
    out = []
    for stmt in filter(None, (s.strip() for s in body.split(";"))):
        if "*" in stmt:
            out.append((re.search(r"(\w+)$", stmt).group(1), C.c_void_p))
        else:
            kind, names = (stmt.split(None, 1) + [""])[:2]
            out += [(n.strip(), _scalar([kind, n.strip()], where)) for n in names.split(",")]
    return out


def _param(text, structs, where):
    words = text.replace("*", " * ").split()
    if "*" not in words:
        return _scalar(words, where)
    base = [w for w in words[:-1] if w != "const"]
    if base == ["char", "*"] and words[0] == "const":
        return C.c_char_p
    if len(base) == 2 and base[0] in structs:
        return C.POINTER(structs[base[0]])
    return C.c_void_p


def parse(text):
    """header text -> (defines {NAME: int}, structs {c name: Structure class}, signatures {name: (restype, argtypes)} in header order)"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines = {m[1]: int(m[2]) for m in re.finditer(r"^#define\s+(SP_\w+)\s+\(?(-?\d+)\)?\s*$", text, flags=re.M)}
    if len(defines) != len(re.findall(r"^#define\s+SP_", text, flags=re.M)):
        raise ValueError("a `#define SP_...` is not `SP_NAME integer` or `SP_NAME (-integer)`, or is repeated (scanpaths_amd/_abi.py)")
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", text):
        structs[m[1]] = type(m[1], (C.Structure,), {"_fields_": _fields(m[2], f"struct {m[1]}")})
    signatures = {}
    for m in re.finditer(r"\b(int64_t|int)\s+(sp_\w+)\s*\(([^;{}()]*)\)\s*;", text):
        args = [] if m[3].strip() in ("", "void") else m[3].split(",")
        signatures[m[2]] = (SCALARS[m[1]], [_param(a, structs, m[2]) for a in args])
    stray = sorted(set(re.findall(r"\b(sp_\w+)\s*\(", text)) - set(signatures))
    if stray:
        raise ValueError(f"{stray}: followed by `(` but not read as `int|int64_t name(args);` declarations (scanpaths_amd/_abi.py)")
    return defines, structs, signatures


def load(path=HEADER_PATH):
    if not os.path.exists(path):
        raise RuntimeError(f"{path} is missing: the ctypes binding is read from this header, which ships beside the package "
                           "as scanpaths_amd/csrc/common.h includes it.  There is no second copy of the ABI.")
    with open(path) as f:
        return parse(f.read())
