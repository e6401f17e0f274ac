"""The suite's one reading of include/scanpaths_amd.h and its one loader of the built library (a plain helper module).

header_decls() is the SECOND OPINION on the binding: scanpaths_amd/_abi.py derives hip.SIGNATURES from the same header, so this reading
shares no code with it.  Every per-feature CPU test states its entry points as NEW = {name: (return type, argument count)} and hands
them to assert_declared(); tests/test_cpu_host.py holds all of hip.SIGNATURES to header_decls() with assert_bound()."""
import ctypes
import os
import re
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scanpaths_amd.h")
KINDS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "double": ctypes.c_double, "float": ctypes.c_float}
DESCRIPTORS = {"sp_conv_desc": "ConvDesc", "sp_wgrad_desc": "WgradDesc"}     # C struct -> the class scanpaths_amd.hip exposes it as


def header_text():
    """the header without its comments"""
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def header_symbols():
    return sorted(set(re.findall(r"\b(sp_[A-Za-z0-9_]+)\s*\(", header_text())))


def header_decls():
    """name -> (return type, [argument strings, white space normalised]) of every `int|int64_t sp_name(...);`"""
    decls = {}
    for m in re.finditer(r"\b(int64_t|int)\s+(sp_[A-Za-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header_text(), flags=re.S):
        ret, name, args = m.group(1), m.group(2), " ".join(m.group(3).split())
        decls[name] = (ret, [] if args in ("", "void") else [a.strip() for a in args.split(",")])
    return decls


def header_abi_version():
    return int(re.search(r"#define SP_ABI_VERSION (\d+)", header_text()).group(1))


def raw_lib():
    """the built library (built first if missing) with every entry point typed by hip.bind; no device is touched"""
    from scanpaths_amd import hip
    if not os.path.exists(hip.LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.bind(ctypes.CDLL(hip.LIB_PATH))


def exported_functions():
    """the sp_* functions the built library defines and exports, read from its ELF64 .dynsym (not through the binding)"""
    raw_lib()
    from scanpaths_amd import hip
    with open(hip.LIB_PATH, "rb") as f:
        data = f.read()
    shoff, = struct.unpack_from("<Q", data, 40)
    shentsize, shnum = struct.unpack_from("<HH", data, 58)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for _, kind, _, _, off, size, link, _, _, entsize in sections:
        if kind == 11:                                                      # SHT_DYNSYM; `link` is its string table
            for at in range(off, off + size, entsize):
                name, info, _, shndx = struct.unpack_from("<IBBH", data, at)
                if info & 15 == 2 and shndx != 0:                           # STT_FUNC, defined here
                    end = data.index(b"\0", sections[link][4] + name)
                    names.add(data[sections[link][4] + name:end].decode())
    return sorted(n for n in names if n.startswith("sp_"))


def want_ctype(arg):
    """the one ctypes type a declared argument may be bound as"""
    from scanpaths_amd import hip
    if "*" not in arg:
        return KINDS[arg.split()[0]]
    words = arg.replace("*", " * ").split()
    if words.count("*") == 1 and words[:3] == ["const", "char", "*"]:
        return ctypes.c_char_p
    if words.count("*") == 1 and words[0] == "const" and words[1] in DESCRIPTORS:
        return ctypes.POINTER(getattr(hip, DESCRIPTORS[words[1]]))
    assert not any(w in DESCRIPTORS for w in words), arg
    return ctypes.c_void_p


def assert_bound(name, decl):
    """hip.SIGNATURES[name] is the declaration `decl` of header_decls(): return type, argument count, every argument's type"""
    from scanpaths_amd import hip
    ret, args = decl
    assert name in hip.SIGNATURES, name
    cret, cargs = hip.SIGNATURES[name]
    assert cret is KINDS[ret], (name, ret, cret)
    assert len(cargs) == len(args), (name, len(cargs), args)
    for a, c in zip(args, cargs):
        assert c is want_ctype(a), (name, a, c)


def assert_declared(expected, prefixes=(), allowed=()):
    """expected {name: (return type, argument count)} is declared in the header so, bound in hip.SIGNATURES to match and exported; no other
    entry point starts with one of `prefixes` but those in `allowed` (no suffixed variants); header, binding and library are ABI version 4.
    Returns the bound library."""
    from scanpaths_amd import hip
    decls, lib = header_decls(), raw_lib()
    for name, (ret, nargs) in expected.items():
        assert name in decls, f"{name} is not declared in include/scanpaths_amd.h"
        assert decls[name][0] == ret and len(decls[name][1]) == nargs, (name, decls[name])
        assert_bound(name, decls[name])
        assert hasattr(lib, name), f"{name} is not exported"
    variants = [n for n in sorted(set(decls) | set(hip.SIGNATURES))
                if prefixes and n.startswith(tuple(prefixes)) and n not in expected and n not in allowed]
    assert not variants, f"no suffixed variants: {variants}"
    assert header_abi_version() == hip.ABI_VERSION == lib.sp_abi_version() == 4
    return lib
