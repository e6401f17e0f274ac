"""CPU-only checks of scanpaths_amd/_abi.py, which derives the ctypes binding (hip.SIGNATURES, hip.ConvDesc, hip.WgradDesc, hip.ABI_VERSION)
from include/scanpaths_amd.h: every rule of the parser on synthetic header text, every refusal, and on the real header
signatures written out by hand (a reader cannot pin its own mistake) -- one entry point of every kind, the descriptor pointers and the
descriptors' layout."""
import ctypes as C

import pytest

import abi
from scanpaths_amd import _abi, hip

_P, _I, _L, _F, _D, _U = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_double, C.c_uint64

SYNTHETIC = """
/* a comment with sp_not_a_call( inside */
#define SP_OK 0
#define SP_EBAD (-7)   /* negative, in parentheses */
#define SP_ABI_VERSION 12
#define NOT_OURS 1.5
typedef struct sp_thing {
    int a, b,
        c;            // a list over two lines
    float alpha;
    int64_t stride; uint64_t seed;
    double eps;
    const int* rows;  /* any pointer field */
    void* work;
} sp_thing;
int sp_none(void);
int sp_empty();
int64_t sp_scalars(int a, int64_t b, uint64_t c, float d, double e);
int sp_pointers(const char* name, const void* const* lists, const float* const* more, unsigned long long* mask, float* out,
                void* stream);
int sp_structs(const sp_thing* d, sp_thing* e, const sp_thing* const* many,
               int n /* a comment between arguments */,
               void* stream);
"""


def test_every_rule_on_synthetic_text():
    defines, structs, sigs = _abi.parse(SYNTHETIC)
    assert defines == {"SP_OK": 0, "SP_EBAD": -7, "SP_ABI_VERSION": 12}
    T = structs["sp_thing"]
    assert list(structs) == ["sp_thing"] and issubclass(T, C.Structure)
    assert T._fields_ == [("a", _I), ("b", _I), ("c", _I), ("alpha", _F), ("stride", _L), ("seed", _U), ("eps", _D), ("rows", _P), ("work", _P)]
    assert T(a=1, eps=0.5, work=None).eps == 0.5                                      # keyword construction, as ConvGeom.fwd_desc does
    assert list(sigs) == ["sp_none", "sp_empty", "sp_scalars", "sp_pointers", "sp_structs"]          # header order
    assert sigs["sp_none"] == (_I, []) and sigs["sp_empty"] == (_I, [])
    assert sigs["sp_scalars"] == (_L, [_I, _L, _U, _F, _D])
    assert sigs["sp_pointers"] == (_I, [C.c_char_p, _P, _P, _P, _P, _P])
    assert sigs["sp_structs"] == (_I, [C.POINTER(T), C.POINTER(T), _P, _I, _P])


@pytest.mark.parametrize("text,names", [
    ("int sp_f(long n);", "sp_f"),                                                    # a scalar the rules do not know
    ("int sp_f(unsigned n);", "sp_f"),
    ("int sp_f(int);", "sp_f"),                                                       # no parameter name
    ("typedef struct sp_t { int a; } sp_t;\nint sp_f(sp_t d);", "sp_f"),              # a struct by value
    ("typedef struct sp_t { long a; } sp_t;", "sp_t"),
    ("typedef struct sp_t { int a[4]; } sp_t;", "sp_t"),
    ("float sp_f(int n);", "sp_f"),                                                   # completeness: not int / int64_t
    ("void sp_f(int n);", "sp_f"),
    ("int sp_f(int n) { return sp_g(n); }", "sp_f"),                                  # a definition, not a declaration
    ("#define SP_CALL sp_x(1)", "SP_"),
    ("static int v = sp_x(1);", "sp_x"),                                              # an sp_x( that is no declaration
    ("#define SP_RATE 1.5", "SP_"),
    ("#define SP_OK 0\n#define SP_OK 1", "SP_"),
])
def test_refusals_name_the_declaration(text, names):
    with pytest.raises(ValueError, match=names):
        _abi.parse(text)


def test_a_missing_header_is_named(tmp_path):
    with pytest.raises(RuntimeError, match="no_such_header.h is missing"):
        _abi.load(str(tmp_path / "no_such_header.h"))
    assert _abi.HEADER_PATH == abi.HEADER


# written by hand from the header, one entry point of every kind ("C" / "W": pointer to ConvDesc / WgradDesc)
PINNED = {
    "sp_abi_version": (_I, []),
    "sp_set_tuning": (_I, [C.c_char_p, _I]),
    "sp_split2_f16_rows": (_I, [_P, _L, _L, _I, _P, _P, _P, _P]),
    "sp_boot_resample": (_I, [_P, _P, _I, _I, _I, _P, _I, _I, _U, _P, _P, _P]),
    "sp_sample_actions": (_I, [_P, _P, _P, _I, _I, _I, _I, _U, _P, _P, _P, _P]),
    "sp_scanmatch_submatrix": (_I, [_I, _I, _D, _P, _P, _P]),
    "sp_clip_adam": (_I, [_P, _P, _P, _P, _L, _P, _F, _F, _F, _F, _F, _F, _F, _F, _F, _P]),
    "sp_conv_wgrad_f16x2_multi_workspace": (_L, ["W", _I]),
    "sp_conv_wgrad_f16x2_multi": (_I, ["W", _I, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "sp_gateconv_lstm_f16x2": (_I, ["C", _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _P, _P, _P, _P, _P, _P, _F, _P]),
    "sp_conv_igemm": (_I, ["C", _P, _P, _P, _P, _P]),
    "sp_bn_fwd_split": (_I, [_P, _L, _I, _F, _F, _P, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _P]),
    "sp_resize_normalize_images": (_I, [_P, _P, _P, _I, _I, _I, _F, _F, _F, _F, _F, _F, _P, _P]),
}
# every entry point that takes a descriptor, and which one
DESCRIPTOR_CALLS = {
    "sp_conv_igemm": "C", "sp_conv_igemm_bf16x3": "C", "sp_conv_igemm_f16x2": "C", "sp_conv_igemm_f16x1": "C", "sp_conv_stats_tiles": "C",
    "sp_conv_igemm_f16x2_stats": "C", "sp_gateconv_lstm_f16x2": "C",
    "sp_conv_wgrad_workspace": "W", "sp_conv_wgrad": "W", "sp_conv_wgrad_bf16x3_workspace": "W", "sp_conv_wgrad_bf16x3": "W",
    "sp_conv_wgrad_f16x2_workspace": "W", "sp_conv_wgrad_f16x2": "W", "sp_conv_wgrad_f16x2_multi_workspace": "W",
    "sp_conv_wgrad_f16x2_multi": "W", "sp_conv_wgrad_f16x1": "W",
}


def _desc(tag):
    return {"C": C.POINTER(hip.ConvDesc), "W": C.POINTER(hip.WgradDesc)}.get(tag, tag)


def test_the_real_header_gives_the_pinned_signatures():
    assert len(hip.SIGNATURES) == 154 and list(hip.SIGNATURES) == list(abi.header_decls())
    for name, (res, args) in PINNED.items():
        assert hip.SIGNATURES[name] == (res, [_desc(a) for a in args]), name
    assert hip.ABI_VERSION == 4 and hip._DEFINES == {"SP_OK": 0, "SP_EINVAL": -1, "SP_ENULL": -2, "SP_ABI_VERSION": 4}
    with pytest.raises(hip.HipError, match="SP_EINVAL"):
        hip.check(-1, "x")
    with pytest.raises(hip.HipError, match="SP_ENULL"):
        hip.check(-2, "x")
    with pytest.raises(hip.HipError, match="hipError 700"):
        hip.check(700, "x")
    hip.check(0, "x")


def test_descriptor_pointers_are_typed_everywhere():
    """a descriptor goes in position 0 as POINTER of its own class and nowhere else; a bare address or the other descriptor is refused
    by ctypes before the call"""
    takes = {n: a for n, (_, a) in hip.SIGNATURES.items() if any(issubclass(t, C._Pointer) for t in a)}
    assert sorted(takes) == sorted(DESCRIPTOR_CALLS)
    for name, tag in DESCRIPTOR_CALLS.items():
        assert takes[name][0] is _desc(tag), name
        assert not any(issubclass(t, C._Pointer) for t in takes[name][1:]), name
    wgrad_ws = abi.raw_lib().sp_conv_wgrad_f16x2_workspace
    for bad in (C.byref(hip.ConvDesc()), C.addressof(hip.WgradDesc()), C.c_void_p(4096)):
        with pytest.raises(C.ArgumentError):
            wgrad_ws(bad)


def test_descriptor_layout():
    """sizes and offsets as the C compiler lays the two structs out on x86-64, written by hand"""
    cd, wd = hip.ConvDesc, hip.WgradDesc
    assert C.sizeof(cd) == 144 and C.sizeof(wd) == 120
    assert [n for n, _ in cd._fields_] == ["N_img", "Hi", "Wi", "Kc", "ldx", "Ho", "Wo", "Nout", "ldc", "KH", "KW", "stride", "pad", "dil", "mode",
                                          "ldw", "alpha", "beta", "relu", "nbatch", "strideX", "strideW", "strideC", "ksplit", "workspace",
                                          "w_scale_rows", "row_last", "row_step"]
    assert [n for n, _ in wd._fields_] == ["N_img", "Hi", "Wi", "Ci", "ldx", "Ho", "Wo", "Co", "ldy", "KH", "KW", "stride", "pad", "dil", "ldo",
                                          "beta", "alpha", "nbatch", "strideX", "strideY", "strideO", "x_scale_vec", "y_scale_vec", "row_last",
                                          "row_step"]
    assert (cd.alpha.offset, cd.strideX.offset, cd.workspace.offset, cd.row_last.offset, cd.row_step.offset) == (64, 80, 112, 128, 136)
    assert (wd.alpha.offset, wd.strideX.offset, wd.x_scale_vec.offset, wd.row_last.offset, wd.row_step.offset) == (64, 72, 96, 104, 112)
    assert dict(cd._fields_)["alpha"] is _F and dict(cd._fields_)["strideX"] is _L and dict(cd._fields_)["workspace"] is _P
    assert dict(wd._fields_)["alpha"] is _F and dict(wd._fields_)["strideO"] is _L and dict(wd._fields_)["row_last"] is _P
    d = hip.ConvDesc(N_img=2, alpha=0.5, strideX=1 << 40, workspace=None, row_step=7)
    assert (d.N_img, d.alpha, d.strideX, d.workspace, d.row_step) == (2, 0.5, 1 << 40, None, 7)
