"""The suite's reading of include/scanpaths_amd_model.h and of the exports of libscanpaths_amd_model.so (a plain helper module beside
tests/abi.py and tests/stats_abi.py, which read the other two headers and libraries).  It shares no code with scanpaths_amd/_abi.py,
from which hip.MODEL_SIGNATURES is derived; the ELF reader and the ctypes kinds are stats_abi's."""
import ctypes
import os
import re

from stats_abi import KINDS, exported_functions, want_ctype  # noqa: F401

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "scanpaths_amd_model.h")


def header_text():
    """the header without its comments"""
    with open(HEADER) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def header_comment():
    """the header's comments alone"""
    with open(HEADER) as f:
        return " ".join(" ".join(re.findall(r"/\*.*?\*/", f.read(), flags=re.S)).replace("*", " ").split())


def header_decls():
    """name -> (return type, [argument strings]) of every `int|int64_t sp_name(...);`"""
    decls = {}
    for m in re.finditer(r"\b(int64_t|int)\s+(sp_[A-Za-z0-9_]+)\s*\(([^;{]*?)\)\s*;", header_text(), flags=re.S):
        args = " ".join(m.group(3).split())
        decls[m.group(2)] = (m.group(1), [] if args in ("", "void") else [a.strip() for a in args.split(",")])
    return decls


def header_version():
    return int(re.search(r"#define SP_MODEL_ABI_VERSION (\d+)", header_text()).group(1))


def lib_path():
    """the built model library (everything is built first if it is missing)"""
    from scanpaths_amd import hip
    if not os.path.exists(hip.MODEL_LIB_PATH):
        import __graft_entry__ as g
        g.build()
    return hip.MODEL_LIB_PATH


def raw_lib():
    """the model library with every entry point typed from hip.MODEL_SIGNATURES; no device is touched"""
    from scanpaths_amd import hip
    cdll = ctypes.CDLL(lib_path())
    for name, (restype, argtypes) in hip.MODEL_SIGNATURES.items():
        fn = getattr(cdll, name)
        fn.restype, fn.argtypes = restype, argtypes
    return cdll
