"""The 3xbf16 kernels of csrc/conv_bf16x3.hip through the C ABI -- sp_split3_bf16, sp_split3_bf16_wT, sp_conv_igemm_bf16x3 (forward and data
gradient), sp_conv_wgrad_bf16x3 with its workspace query and slab reducer -- against tests/bf16x3_ref.py (held to torch's bf16 conversion, its
fp64 conv and autograd and to its own claims by tests/test_bf16x3_ref_cpu.py).

Splitters: bit equality of planes and zero block with the numpy restatement, between guards of bf16 NaNs that must survive.  GEMMs: the operands
are what the DEVICE splitters wrote (checked against the restatement first, still between their NaN guards; the fp32 sources between NaN guards
too), outputs and workspaces lie in parity.Guarded allocations whose pads (ldc > Nout, ldo > Ntot), gaps and guards hold a sentinel word and
must be unchanged after the launch, workspaces are exactly the queried size.  Every case runs on Gaussian data -- every live word finite and inside
the ELEMENT-WISE derived bar against R_planes (bf16x3_ref: chain_b3, chain_w3), inside rep_bound plus that bar against R_true, and inside the
2e-6 max-norm bar of tests/test_ops_gpu.py -- and on LATTICE data, where every summation order is exact and the kernel must equal R_planes word
for word.  Slab launches run twice and give identical bits.  Each comparison prints a PARITY line, the module a summary per group
(profiles/conv_bf16x3_parity.md).  Out of scope here: the timing-library modes of b3_kernel, operands past 2^32 bytes (only their refusal),
subnormal planes."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bf16x3_ref as R
import parity as P

pytestmark = pytest.mark.gpu

EINVAL, ENULL = -1, -2
LEGACY = 2e-6                   # the max-norm bar of tests/test_ops_gpu.py for these kernels
HG = 128                        # bf16 NaNs before and after a split operand (256 bytes: the 16-byte alignment is kept)
SUM = P.Summary("bf16x3", ("bf16x3_igemm_gemm", "bf16x3_igemm_epilogue", "bf16x3_igemm_conv", "bf16x3_wgrad_gemm", "bf16x3_wgrad_maps",
                           "bf16x3_wgrad_splits"))
_summary = SUM.fixture()
_b3, _w3 = functools.lru_cache(maxsize=None)(R.B3Problem), functools.lru_cache(maxsize=None)(R.W3Problem)


# ====================================================================================================================
# splitters
# ====================================================================================================================
class Planes:
    """where a device splitter writes: n halves, every one a bf16 NaN before the launch, between HG bf16 NaNs on either side"""
    def __init__(self, n):
        self.n = n
        self.dev = torch.from_numpy(np.full(2 * HG + n, R.BF16_QNAN, np.uint16).view(np.int16)).to(P.dev())
        self.ptr = self.dev.data_ptr() + 2 * HG

    def read(self, what):
        a = self.dev.cpu().numpy().view(np.uint16)
        assert (a[:HG] == R.BF16_QNAN).all() and (a[HG + self.n:] == R.BF16_QNAN).all(), f"{what}: a guard of the split operand changed"
        return a[HG:HG + self.n]

    def untouched(self):
        return bool((self.dev.cpu().numpy().view(np.uint16) == R.BF16_QNAN).all())


def _planes_equal(got, want, what):
    assert got.size == want.size, (what, got.size, want.size)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} halves differ, first at {bad[0]}: {got[bad[0]]:#06x} != {want[bad[0]]:#06x}"


def _split(x, want, what, wT=None):
    """one launch of a device splitter on a source between NaN guards -> the Planes it wrote, equal to the restatement bit for bit"""
    hip, L = P.abi()
    src = P.operand(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)))
    out = Planes(want.size)
    if wT is None:
        rc = L.sp_split3_bf16(src.ptr, x.size, out.ptr, hip.stream())
    else:
        rc = L.sp_split3_bf16_wT(src.ptr, *wT, out.ptr, hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)
    assert src.untouched()
    _planes_equal(out.read(what), want, what)
    return out


def _split_data(n, seed):
    x = R.wide(n, seed)
    x[::7] = 0
    x[3::16] = -0.0
    x[5::16] = R.gauss((x[5::16].size,), seed + 1)
    return x


@pytest.mark.parametrize("n", [16, 48, 4096 * 256 * 4 + 16], ids=["n16", "n48", "two-passes"])
def test_split3_bf16(n):
    x = _split_data(n, n)
    want = R.split3_bf16(x)
    assert want.size == 3 * n + 32
    _split(x, want, f"split3 n={n}")


@pytest.mark.parametrize("Co,taps,Ci", [(16, 1, 16), (48, 9, 16), (16, 9, 130), (272, 1, 128)])
def test_split3_bf16_wT(Co, taps, Ci):
    w = _split_data(Co * taps * Ci, Co + taps + Ci).reshape(Co, taps, Ci)
    _split(w, R.split3_bf16_wT(w), f"wT {Co} {taps} {Ci}", wT=(Co, taps, Ci))


SPLIT_REFUSALS = [("x-null", "sp_split3_bf16", lambda x, o: (None, 32, o), ENULL), ("out-null", "sp_split3_bf16", lambda x, o: (x, 32, None), ENULL),
                  ("n%16", "sp_split3_bf16", lambda x, o: (x, 40, o), EINVAL),
                  ("wT-w-null", "sp_split3_bf16_wT", lambda x, o: (None, 16, 1, 4, o), ENULL),
                  ("wT-out-null", "sp_split3_bf16_wT", lambda x, o: (x, 16, 1, 4, None), ENULL),
                  ("wT-tapsCo%16", "sp_split3_bf16_wT", lambda x, o: (x, 8, 3, 4, o), EINVAL)]


@pytest.mark.parametrize("name,fn,args,rc", SPLIT_REFUSALS, ids=[r[0] for r in SPLIT_REFUSALS])
def test_splitter_refusals(name, fn, args, rc):
    hip, L = P.abi()
    x, out = P.operand(torch.ones(256)), Planes(3 * 256 + 32)
    assert getattr(L, fn)(*args(x.ptr, out.ptr), hip.stream()) == rc, name
    torch.cuda.synchronize()
    assert out.untouched() and x.untouched(), f"{name}: a refused call wrote"


# ====================================================================================================================
# sp_conv_igemm_bf16x3
# ====================================================================================================================
def _b3_out(p):
    return P.Guarded(1, p.M, p.c.Nout, p.ldc, fill="sentinel", data=p.out0)


def _b3_desc(hip, p, **kw):
    c = p.c
    a = dict(N_img=c.N_img, Hi=c.Hi, Wi=c.Wi, Kc=c.Kc, ldx=c.Kc, Ho=c.Ho, Wo=c.Wo, Nout=c.Nout, ldc=p.ldc, KH=c.KH, KW=c.KW, stride=c.stride, pad=c.pad,
             dil=c.dil, mode=c.mode, ldw=p.K if c.mode == 0 else c.Nout, alpha=c.alpha, beta=c.beta, relu=int(c.relu), nbatch=1)
    a.update(kw)
    return hip.ConvDesc(**a)


def _launch_b3(p, *, null=(), off=None, desc=None, expect=0):
    """one launch on fresh buffers, the operands from the device splitters -> the output allocation on the host"""
    hip, L = P.abi()
    c = p.c
    off = off or {}
    name = f"{c.name} [{p.kind}]"
    dX = _split(p.x, p.Xp, name + " X")
    dW = _split(p.w, p.Wp, name + " W") if c.mode == 0 else _split(p.w, p.Wp, name + " W^T", wT=(c.Kc, c.KH * c.KW, c.Nout))
    out = _b3_out(p)
    dO, dB = P.up(out), P.operand(p.bias)
    d = _b3_desc(hip, p, **(desc or {}))
    ptr = {"X": dX.ptr + off.get("X", 0), "W": dW.ptr + off.get("W", 0), "bias": P.at(dB), "out": P.at(dO)}
    for k in null:
        ptr[k] = None
    rc = L.sp_conv_igemm_bf16x3(ctypes.byref(d), ptr["X"], ptr["W"], ptr["bias"], ptr["out"], hip.stream())
    torch.cuda.synchronize()
    assert rc == expect, (c.name, rc, expect)
    dX.read(name + " X after the launch"), dW.read(name + " W after the launch")
    flat = dO.flat()
    if expect != 0:
        assert out.all_untouched(flat), f"{c.name}: a refused call wrote to the output"
    return flat


def _check(group, p, out, flat, name):
    """one launch against R_planes (guards, finiteness, the element-wise bar, the max-norm bar; exactly on lattice data) and against R_true
    (rep_bound plus the bar, and the max-norm bar)"""
    ref, S = p.planes()
    SUM.judge(group, name, out, flat, ref, S, p.chain, LEGACY)
    got, true = out.live(flat).double(), p.true()
    assert ((got - true).abs() <= p.rep_bar() + P.bar(S, p.chain)).all(), f"{name}: outside the representation bound of the true product"
    P.close(got, true, LEGACY, name)
    if p.kind == "lattice":
        assert p.exact_span() <= 2.0 ** 24
        SUM.exact(group, name, got, ref)


def _run_b3(group, case, kinds=("gauss", "lattice")):
    for kind in kinds:
        p = _b3(case, kind)
        _check(group, p, _b3_out(p), _launch_b3(p), f"{case.name} [{kind}] (nkt {p.K // 16}, c {p.chain})")


@pytest.mark.parametrize("case", R.b3_gemm_cases(), ids=lambda c: c.name)
def test_igemm_as_gemm(case):
    _run_b3("bf16x3_igemm_gemm", case, ("gauss", "lattice", "heavy") if "mode0-nkt" in case.name else ("gauss", "lattice"))


@pytest.mark.parametrize("case", R.b3_epilogue_cases(), ids=lambda c: c.name)
def test_igemm_epilogue(case):
    _run_b3("bf16x3_igemm_epilogue", case)


@pytest.mark.parametrize("case", R.b3_conv_cases(), ids=lambda c: c.name)
def test_igemm_as_conv(case):
    _run_b3("bf16x3_igemm_conv", case)


_G = R._bg("refusal-gemm", 256, 32, 64, 0, ldc_pad=0)
B3_REFUSALS = [
    ("X-null", dict(null=("X",)), ENULL), ("W-null", dict(null=("W",)), ENULL), ("out-null", dict(null=("out",)), ENULL),
    ("mode2", dict(desc=dict(mode=2)), EINVAL), ("Kc%16", dict(desc=dict(Kc=24, ldx=24)), EINVAL), ("ldx!=Kc", dict(desc=dict(ldx=48)), EINVAL),
    ("X+8B", dict(off=dict(X=8)), EINVAL), ("W+8B", dict(off=dict(W=8)), EINVAL), ("nbatch2", dict(desc=dict(nbatch=2)), EINVAL),
    ("nbatch0", dict(desc=dict(nbatch=0)), EINVAL), ("stride0", dict(desc=dict(stride=0)), EINVAL), ("dil0", dict(desc=dict(dil=0)), EINVAL),
    ("Nout0", dict(desc=dict(Nout=0)), EINVAL), ("M0", dict(desc=dict(N_img=0)), EINVAL),
    ("X-past-2^32-bytes", dict(desc=dict(N_img=1, Hi=8192, Wi=8192, Kc=16, ldx=16)), EINVAL),
    ("W-past-2^32-bytes", dict(desc=dict(Nout=1 << 20, KH=7, KW=7, Kc=16, ldx=16)), EINVAL),
]


@pytest.mark.parametrize("name,how,rc", B3_REFUSALS, ids=[r[0] for r in B3_REFUSALS])
def test_igemm_refusals(name, how, rc):
    """the code the header states, before anything is launched: the output stays all-sentinel"""
    _launch_b3(_b3(_G, "gauss"), expect=rc, **how)


# ====================================================================================================================
# sp_conv_wgrad_bf16x3
# ====================================================================================================================
def _w3_out(p):
    return P.Guarded(1, p.c.Co, p.Ntot, p.ldo, fill="sentinel", data=p.out0)


def _w3_desc(hip, p, **kw):
    c = p.c
    a = dict(N_img=c.N_img, Hi=c.Hi, Wi=c.Wi, Ci=c.Ci, ldx=c.Ci, Ho=c.Ho, Wo=c.Wo, Co=c.Co, ldy=c.Co, KH=c.KH, KW=c.KW, stride=c.stride, pad=c.pad,
             dil=c.dil, ldo=p.ldo, beta=c.beta, alpha=c.alpha, nbatch=1)
    a.update(kw)
    return hip.WgradDesc(**a)


@functools.lru_cache(maxsize=4)
def _w3_operands(p):
    name = f"{p.c.name} [{p.kind}]"
    return _split(p.x, p.Xp, name + " X"), _split(p.dy, p.Yp, name + " dY")


def _launch_w3(p, *, null=(), off=None, desc=None, expect=0):
    hip, L = P.abi()
    c = p.c
    off = off or {}
    dX, dY = _w3_operands(p)
    out = _w3_out(p)
    dO = P.up(out)
    d = _w3_desc(hip, p, **(desc or {}))
    nbytes = L.sp_conv_wgrad_bf16x3_workspace(ctypes.byref(d))
    if desc is None:
        assert nbytes == R.w3_workspace(p.M, c.Co, p.Ntot, p.ldo) == (p.splits * c.Co * p.ldo * 4 if p.splits > 1 else 0), (c.name, nbytes, p.splits)
    dWs = P.output(nbytes // 4) if nbytes else None          # exactly the queried size between sentinels
    ptr = {"X": dX.ptr + off.get("X", 0), "Y": dY.ptr + off.get("Y", 0), "out": P.at(dO), "ws": P.at(dWs)}
    for k in null:
        ptr[k] = None
    rc = L.sp_conv_wgrad_bf16x3(ctypes.byref(d), ptr["X"], ptr["Y"], ptr["out"], ptr["ws"], hip.stream())
    torch.cuda.synchronize()
    assert rc == expect, (c.name, rc, expect)
    dX.read(c.name + " X after the launch"), dY.read(c.name + " dY after the launch")
    flat = dO.flat()
    if dWs is not None:
        assert dWs.pads_untouched(), f"{c.name}: a word around the slab workspace changed"
        assert expect == 0 or dWs.untouched()
    if expect != 0:
        assert out.all_untouched(flat), f"{c.name}: a refused call wrote to the output"
    return flat


def _run_w3(group, case, kinds=("gauss", "lattice")):
    for kind in kinds:
        p = _w3(case, kind)
        flat = _launch_w3(p)
        _check(group, p, _w3_out(p), flat, f"{case.name} [{kind}] (splits {p.splits}, c {p.chain})")
        if p.splits > 1:
            assert P.same_bits(flat, _launch_w3(p)), f"{case.name}: two slab launches differ"


@pytest.mark.parametrize("case", R.w3_gemm_cases(), ids=lambda c: c.name)
def test_wgrad_as_gemm(case):
    """Ho = Wo = 1 with N_img = rows: a 16-pixel K-tile crosses 16 images"""
    _run_w3("bf16x3_wgrad_gemm", case, ("gauss", "lattice", "heavy") if case.name.startswith("rows") else ("gauss", "lattice"))


@pytest.mark.parametrize("case", R.w3_map_cases(), ids=lambda c: c.name)
def test_wgrad_maps(case):
    _run_w3("bf16x3_wgrad_maps", case)


@pytest.mark.parametrize("case", R.w3_split_cases(), ids=lambda c: c.name)
def test_wgrad_splits(case):
    _run_w3("bf16x3_wgrad_splits", case)


def test_wgrad_at_the_cap_of_64_splits():
    p = _w3(R.W3_CAP, "gauss")
    assert p.splits == 64
    _run_w3("bf16x3_wgrad_splits", R.W3_CAP)


_W = R._wg("refusal-wgrad", 64, 32, 128, ldo_pad=0)
_WS = R._wg("refusal-wgrad-slabs", 1024, 16, 128)
W3_REFUSALS = [
    ("X-null", _W, dict(null=("X",)), ENULL), ("dY-null", _W, dict(null=("Y",)), ENULL), ("dW-null", _W, dict(null=("out",)), ENULL),
    ("Ci%128", _W, dict(desc=dict(Ci=64, ldx=64)), EINVAL), ("Co%16", _W, dict(desc=dict(Co=24, ldy=24)), EINVAL),
    ("ldx!=Ci", _W, dict(desc=dict(ldx=256)), EINVAL), ("ldy!=Co", _W, dict(desc=dict(ldy=48)), EINVAL), ("nbatch2", _W, dict(desc=dict(nbatch=2)), EINVAL),
    ("X+8B", _W, dict(off=dict(X=8)), EINVAL), ("dY+8B", _W, dict(off=dict(Y=8)), EINVAL), ("M0", _W, dict(desc=dict(N_img=0)), EINVAL),
    ("X-past-2^32-bytes", _W, dict(desc=dict(N_img=1, Hi=4096, Wi=4096)), EINVAL),
    ("slabs-workspace-null", _WS, dict(null=("ws",)), ENULL),
]


@pytest.mark.parametrize("name,case,how,rc", W3_REFUSALS, ids=[r[0] for r in W3_REFUSALS])
def test_wgrad_refusals(name, case, how, rc):
    """the output and the workspace (exactly the queried size, where the query gives one) stay all-sentinel"""
    _launch_w3(_w3(case, "gauss"), expect=rc, **how)
