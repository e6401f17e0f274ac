"""The suite's reading of include/scanpaths_amd_stats.h and of the exports of libscanpaths_amd_stats.so (a plain helper module beside
tests/abi.py, which reads only the main header and the main library).  Like abi.header_decls() it shares no code with
scanpaths_amd/_abi.py, from which hip.STATS_SIGNATURES is derived."""
import ctypes
import os
import re
import struct

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scanpaths_amd_stats.h")
KINDS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "double": ctypes.c_double, "float": ctypes.c_float}


def header_text():
    """the header without its comments"""
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def header_decls():
    """name -> (return type, [argument strings]) of every `int|int64_t sp_name(...);`"""
    decls = {}
    for m in re.finditer(r"\b(int64_t|int)\s+(sp_[A-Za-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header_text(), flags=re.S):
        args = " ".join(m.group(3).split())
        decls[m.group(2)] = (m.group(1), [] if args in ("", "void") else [a.strip() for a in args.split(",")])
    return decls


def header_version():
    return int(re.search(r"#define SP_STATS_ABI_VERSION (\d+)", header_text()).group(1))


def want_ctype(arg):
    """the one ctypes type a declared argument may be bound as: a pointer is a void pointer, a scalar its own kind"""
    return ctypes.c_void_p if "*" in arg else KINDS[arg.split()[0]]


def lib_path():
    """the built stats library (everything is built first if it is missing)"""
    from scanpaths_amd import hip
    if not os.path.exists(hip.STATS_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.STATS_LIB_PATH


def raw_lib():
    """the stats library with every entry point typed from hip.STATS_SIGNATURES; no device is touched"""
    from scanpaths_amd import hip
    cdll = ctypes.CDLL(lib_path())
    for name, (restype, argtypes) in hip.STATS_SIGNATURES.items():
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = restype, argtypes
    return cdll


def exported_functions(path):
    """the sp_* functions an ELF64 shared library defines and exports, read from its .dynsym"""
    with open(path, "rb") as f:
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
