"""The 2xfp16 kernels of csrc/conv_f16x2.hip through the C ABI -- the five operand splitters, sp_conv_igemm_f16x2 (every h2_kernel build the product
library selects: forward / data gradient, tap-major / channel-block-major / halo, batched, row-sparse, fused statistics), sp_conv_wgrad_f16x2
(hw_kernel, both slab reducers, batched), sp_conv_wgrad_f16x2_multi (hw2_kernel) and the one-product entries -- against tests/f16x2_ref.py (held to
torch's fp64 conv and autograd and to its own claims by tests/test_f16x2_ref_cpu.py).

Splitters: bit equality of planes, zero block and scales with the numpy emulation.  GEMMs: the operands are the emulation's planes (wider rows hold
fp16 NaNs in their pad channels), outputs and workspaces lie in parity.Guarded allocations whose pads, gaps and guards hold a sentinel word and
must be unchanged after the launch, workspaces are exactly the queried size.  Every case runs on Gaussian data -- every live word finite and inside
the ELEMENT-WISE derived bar against R_planes (f16x2_ref: chain_*), the max-norm bars of tests/test_ops_gpu.py against R_true on top -- and on
LATTICE data, where every summation order is exact and the kernel must equal R_planes exactly (torch.equal in fp64: bit for bit up to the sign of
a zero).  Some cases add heavy-tailed data.  Each comparison prints a PARITY line, the module a summary per group (profiles/conv_f16x2_parity.md).
Out of scope here: sp_gateconv_lstm_f16x2 (tests/test_lstm_cell_gpu.py), sp_rank1_grads_f16x2 (tests/test_rank1_grads_gpu.py), the bf16x3 kernels
(tests/test_conv_bf16x3_gpu.py), the timing-library variants."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import f16x2_ref as R
import parity as P

pytestmark = pytest.mark.gpu

EINVAL, ENULL = -1, -2
SUM = P.Summary("f16x2")
_summary = SUM.fixture()
_h2, _hw = functools.lru_cache(maxsize=None)(R.H2Problem), functools.lru_cache(maxsize=None)(R.HWProblem)          # (case, kind) -> operands and restatement, built once


# ====================================================================================================================
# splitters
# ====================================================================================================================
def _data(kind, n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    x = (g.standard_normal(n) * np.exp(g.uniform(-10, 0, n))).astype(np.float32)
    if kind == "zeros":
        x[:] = 0
    elif kind == "tiny":
        x *= np.float32(1e-38) / np.abs(x).max()
        x[n // 2] = 1e-38
    elif kind == "huge":
        x *= np.float32(1.0) / np.abs(x).max()
        x = (x * np.float32(3e38)).astype(np.float32)
        x[n // 3] = -3e38
    return x


SPLIT2 = [("n16", 16, "gauss", None), ("n4112", 4112, "gauss", None), ("two-passes", 4096 * 256 * 4 + 1040, "gauss", None), ("zeros", 1024, "zeros", None),
          ("max-1e-38", 1024, "tiny", None), ("max-3e38", 1024, "huge", None), ("have-amax-1x", 4112, "gauss", 1.0), ("have-amax-7x", 4112, "gauss", 7.0)]


def _planes_equal(got_words, want_u16, what):
    got = got_words.view(np.uint16)
    assert got.size == want_u16.size, (what, got.size, want_u16.size)
    bad = np.nonzero(got != want_u16)[0]
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} halves differ, first at {bad[0]}: {got[bad[0]]:#06x} != {want_u16[bad[0]]:#06x}"


@pytest.mark.parametrize("name,n,kind,bound", SPLIT2, ids=[s[0] for s in SPLIT2])
def test_split2_f16(name, n, kind, bound):
    hip, L = P.abi()
    x = _data(kind, n, P.seed_of(name))
    b = None if bound is None else np.float32(bound) * np.abs(x).max()
    want, s = R.split2_f16(x, bound=b)
    dx, out = P.f32(x), P.raw(4 * n + 64)
    sa = P.raw(8, init=np.array([np.float32(np.nan), np.float32(0.0) if b is None else b], dtype=np.float32))      # {scale, max|x| bits: zero or the bound}
    assert L.sp_split2_f16(dx.data_ptr(), n, out.ptr, sa.ptr, 0 if b is None else 1, hip.stream()) == 0
    torch.cuda.synchronize()
    got_s = sa.read().view(np.float32)
    assert got_s[0] == s, (got_s, s)
    if b is None:
        assert got_s[1] == np.abs(x).max()
    _planes_equal(out.read(), want, name)


@pytest.mark.parametrize("Co,taps,Ci", [(16, 1, 4), (48, 9, 36), (16, 9, 4), (48, 1, 36)])
def test_split2_f16_wT(Co, taps, Ci):
    hip, L = P.abi()
    w = _data("gauss", Co * taps * Ci, Co + taps + Ci).reshape(Co, taps, Ci)
    want, s = R.split2_f16_wT(w)
    dw, out, sa = P.f32(w), P.raw(4 * w.size + 64), P.raw(8, init=np.zeros(2, np.float32))
    assert L.sp_split2_f16_wT(dw.data_ptr(), Co, taps, Ci, out.ptr, sa.ptr, hip.stream()) == 0
    torch.cuda.synchronize()
    assert sa.read().view(np.float32)[0] == s
    _planes_equal(out.read(), want, f"wT {Co} {taps} {Ci}")


@pytest.mark.parametrize("rows,K,Kc,absorb", [(1, 16, 16, False), (3, 288, 32, False), (1, 288, 32, True), (3, 16, 16, True), (3, 288, 96, True)])
def test_split2_f16_rows(rows, K, Kc, absorb):
    hip, L = P.abi()
    g = np.random.Generator(np.random.PCG64(rows * K))
    w = _data("gauss", rows * K, rows + K).reshape(rows, K)
    if rows > 1:
        w[1] = 0                                                       # a row of zeros: scale 1
    ab = None
    if absorb:
        ab = (2.0 ** g.integers(-6, 7, Kc)).astype(np.float32)
        ab[Kc // 2] = 2.0 ** -30
    want, s = R.split2_f16_rows(w, Kc, ab)
    dw, dab, out, sc = P.f32(w), (None if ab is None else P.f32(ab)), P.raw(4 * w.size + 64), P.raw(4 * rows)
    assert L.sp_split2_f16_rows(dw.data_ptr(), rows, K, Kc, None if ab is None else dab.data_ptr(), out.ptr, sc.ptr, hip.stream()) == 0
    torch.cuda.synchronize()
    assert (sc.read().view(np.float32) == s).all()
    _planes_equal(out.read(), want, f"rows {rows} {K} {Kc} {absorb}")


@pytest.mark.parametrize("nbatch,Ci,absorb", [(1, 4, False), (3, 12, False), (3, 20, True), (1, 20, True)])
def test_split2_f16_wT_rows(nbatch, Ci, absorb):
    hip, L = P.abi()
    Co, taps = 16, 3
    g = np.random.Generator(np.random.PCG64(nbatch * Ci))
    w = _data("gauss", nbatch * Co * taps * Ci, nbatch + Ci).reshape(nbatch, Co, taps, Ci)
    w[-1, :, :, Ci - 1] = 0                                            # a row of zeros
    ab = (2.0 ** g.integers(-6, 7, Co)).astype(np.float32) if absorb else None
    want, s = R.split2_f16_wT_rows(w, ab)
    dw, dab, out, sc = P.f32(w), (None if ab is None else P.f32(ab)), P.raw(4 * w.size + 64), P.raw(4 * nbatch * Ci)
    assert L.sp_split2_f16_wT_rows(dw.data_ptr(), nbatch, Co, taps, Ci, None if ab is None else dab.data_ptr(), out.ptr, sc.ptr, hip.stream()) == 0
    torch.cuda.synchronize()
    got_s = sc.read().view(np.float32)
    assert (got_s == s).all() and got_s[-1] == 1.0
    _planes_equal(out.read(), want, f"wT_rows {nbatch} {Ci} {absorb}")


@pytest.mark.parametrize("rows,C", [(1, 16), (5, 16), (5, 272), (1, 1040), (5, 1040), (512 * 64 * 4 + 3, 16)])
def test_split2_f16_cols(rows, C):
    hip, L = P.abi()
    g = np.random.Generator(np.random.PCG64(rows + C))
    x = _data("gauss", rows * C, rows * C).reshape(rows, C) * (2.0 ** g.integers(-8, 9, C)).astype(np.float32)
    x[:, C // 3] = 0                                                   # a dead channel: scale 2^100
    want, s = R.split2_f16_cols(x)
    nbytes = L.sp_split2_f16_cols_workspace(rows, C)
    assert nbytes == R.colamax_blocks(rows, C) * C * 4
    dx, out, sc, scratch = P.f32(x), P.raw(4 * x.size + 64), P.raw(4 * C), P.raw(nbytes)
    assert L.sp_split2_f16_cols(dx.data_ptr(), rows, C, out.ptr, sc.ptr, scratch.ptr, hip.stream()) == 0
    torch.cuda.synchronize()
    scratch.read()
    got_s = sc.read().view(np.float32)
    assert (got_s == s).all() and got_s[C // 3] == np.float32(2.0 ** 100)
    _planes_equal(out.read(), want, f"cols {rows} {C}")


# ====================================================================================================================
# sp_conv_igemm_f16x2 / _f16x1 / _stats
# ====================================================================================================================
def _h2_out(p):
    return P.Guarded(p.c.nbatch, p.M, p.c.Nout, p.ldc, p.M * p.ldc, fill="sentinel", data=p.out0)


def _h2_desc(hip, p, **kw):
    c = p.c
    a = dict(N_img=c.N_img, Hi=c.Hi, Wi=c.Wi, Kc=c.Kc, ldx=p.ldx, Ho=c.Ho, Wo=c.Wo, Nout=c.Nout, ldc=p.ldc, KH=c.KH, KW=c.KW, stride=c.stride, pad=c.pad,
             dil=c.dil, mode=c.mode, ldw=p.K, alpha=c.alpha, beta=c.beta, relu=int(c.relu), nbatch=c.nbatch,
             strideX=p.xrows * p.ldx if c.nbatch > 1 else 0, strideW=c.Nout * p.K if c.nbatch > 1 else 0, strideC=p.M * p.ldc if c.nbatch > 1 else 0,
             w_scale_rows=int(c.sw_rows))
    a.update(kw)
    return hip.ConvDesc(**a)


def _launch_h2(p, *, Xp=None, row_last=None, row_step=0, null=(), off=None, desc=None, expect=0):
    """one launch of the entry the case names on fresh buffers -> (output allocation on the host, (st_partial, st_mm) or None)"""
    hip, L = P.abi()
    c = p.c
    off = off or {}
    dX, dW = P.u16(p.Xp if Xp is None else Xp), P.u16(p.Wp)
    dsx, dsw = P.f32(p.sx), P.f32(p.sw)
    out = _h2_out(p)
    dO = P.up(out)
    dB = P.operand(p.bias)
    drl = None if row_last is None else torch.tensor(row_last, dtype=torch.int32, device=P.dev())
    d = _h2_desc(hip, p, row_last=None if drl is None else drl.data_ptr(), row_step=row_step, **(desc or {}))
    ptr = {"X": dX.data_ptr() + off.get("X", 0), "W": dW.data_ptr() + off.get("W", 0), "sx": dsx.data_ptr(), "sw": dsw.data_ptr(),
           "bias": P.at(dB), "out": P.at(dO)}
    st = None
    if c.stats:
        tiles = L.sp_conv_stats_tiles(ctypes.byref(d))
        assert tiles == P.cdiv(p.M, 256)
        st = (P.raw(tiles * 2 * c.Nout * 8), P.raw(tiles * 2 * c.Nout * 4))
        ptr["stp"], ptr["stm"] = st[0].ptr, st[1].ptr
    for k in null:
        ptr[k] = None
    if c.stats:
        rc = L.sp_conv_igemm_f16x2_stats(ctypes.byref(d), ptr["X"], ptr["sx"], ptr["W"], ptr["sw"], ptr["out"], ptr["stp"], ptr["stm"], hip.stream())
    else:
        fn = L.sp_conv_igemm_f16x2 if c.nprod == 3 else L.sp_conv_igemm_f16x1
        rc = fn(ctypes.byref(d), ptr["X"], ptr["sx"], ptr["W"], ptr["sw"], ptr["bias"], ptr["out"], hip.stream())
    torch.cuda.synchronize()
    assert rc == expect, (c.name, rc, expect)
    flat = dO.flat()
    if expect != 0:
        assert out.all_untouched(flat), f"{c.name}: a refused call wrote to the output"
        assert st is None or (st[0].untouched() and st[1].untouched())
    return flat, st


def _check(group, p, out, flat, name, legacy, cols=slice(None)):
    """one launch against R_planes (guards, the element-wise bar, exactly on lattice data) and against R_true (the max-norm bar; with one product
    the representation bar); cols: the columns of the problem that the output has"""
    ref, S = (v[..., cols] for v in p.planes())
    SUM.judge(group, name, out, flat, ref, S, p.chain, legacy)
    got, true = out.live(flat).double(), p.true()[..., cols]
    if p.c.nprod == 3:
        P.close(got, true, legacy, name)
    else:
        assert ((got - true).abs() <= p.rep_bar()[..., cols] + P.bar(S, p.chain)).all(), f"{name}: outside the 2^-11 representation bar of the true product"
    if p.kind == "lattice":
        assert p.exact_span() <= 2.0 ** 24
        SUM.exact(group, name, got, ref)


def _check_h2(group, p, flat):
    _check(group, p, _h2_out(p), flat, f"{p.c.name} [{p.kind}] {p.build}", 2e-6)


def _dead_items(out, flat, dense, dead, held, what):
    """a launch with row_last against the dense one: guards, live items bit for bit, dead items exact zeros (beta 0) or what they held (beta 1)"""
    assert out.pads_untouched(flat)
    got, want = out.live(flat), out.live(dense)
    for i in range(got.shape[0]):
        if i not in dead:
            assert P.same_bits(got[i], want[i]), (*what, i)
        elif held is not None:
            assert P.same_bits(got[i], held[i]), (*what, i)
        else:
            assert (got[i].view(torch.int32) == 0).all(), (*what, i)


def _run_h2(group, case, kinds=("gauss", "lattice")):
    for kind in kinds:
        p = _h2(case, kind)
        flat, st = _launch_h2(p)
        _check_h2(group, p, flat)
    return p, flat, st


def test_lattice_probe_one_tile():
    """one 256 x 128 x 32 tile on lattice data: v_mfma_f32_16x16x32_f16 sums such data exactly inside one instruction (profiles/conv_f16x2_parity.md)"""
    for mode in (0, 1):
        for rich in (False, True):
            _run_h2("f16x2_probe", R._hg(f"probe-256x128x32-mode{mode}-rich{int(rich)}", 256, 32, 128, mode, ldc_pad=0, ldx_pad=0, rich=rich), ("lattice",))


@pytest.mark.parametrize("case", R.h2_gemm_cases(), ids=lambda c: c.name)
def test_igemm_as_gemm(case):
    _run_h2("f16x2_igemm_gemm", case, ("gauss", "lattice", "heavy") if "Kc" in case.name else ("gauss", "lattice"))


@pytest.mark.parametrize("case", R.h2_conv_cases(), ids=lambda c: c.name)
def test_igemm_as_conv(case):
    _run_h2("f16x2_igemm_conv", case, ("gauss", "lattice", "heavy") if "Kc96" in case.name or "seam" in case.name else ("gauss", "lattice"))


@pytest.mark.parametrize("case", R.h2_x1_cases(), ids=lambda c: c.name)
def test_igemm_one_product(case):
    _run_h2("f16x1_igemm", case)


@pytest.mark.parametrize("case", R.h2_stats_cases(), ids=lambda c: c.name)
def test_igemm_stats(case):
    """the output as any other launch; st_partial against the fp64 sums of the kernel's OWN fp32 output at 1e-12, st_mm equal to its min / max,
    rows at or beyond M not counted"""
    for kind in ("gauss", "lattice"):
        p = _h2(case, kind)
        flat, st = _launch_h2(p)
        _check_h2("f16x2_stats", p, flat)
        got = _h2_out(p).live(flat)[0].double()                                                       # [M, Nout]
        tiles = P.cdiv(p.M, 256)
        stp = torch.from_numpy(st[0].read().view(np.float64).reshape(tiles, 2, case.Nout).copy())
        stm = torch.from_numpy(st[1].read().view(np.float32).reshape(tiles, 2, case.Nout).copy())
        for g in range(tiles):
            v = got[g * 256:min(p.M, (g + 1) * 256)]
            assert ((stp[g, 0] - v.sum(0)).abs() <= 1e-12 * v.abs().sum(0) + 1e-300).all(), (case.name, g)
            assert ((stp[g, 1] - (v * v).sum(0)).abs() <= 1e-12 * (v * v).sum(0) + 1e-300).all(), (case.name, g)
            assert torch.equal(stm[g, 0].double(), v.min(0).values) and torch.equal(stm[g, 1].double(), v.max(0).values), (case.name, g)


# ---- batched forward ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.h2_batched_cases(), ids=lambda c: c.name)
def test_igemm_batched_forward_and_dead_items(case):
    """mode 0, nbatch 3, one weight set per item: dense against the reference; with row_last the live items equal the dense launch bit for bit, dead
    items are exact zeros (beta 0; the float4 writer and its scalar tail at ldc % 4 != 0 / Nout % 4 != 0) or left alone (beta 1) -- and their
    operand rows, NaN planes here, are not read"""
    for kind in ("gauss", "lattice"):
        p = _h2(case, kind)
        dense, _ = _launch_h2(p)
        _check_h2("f16x2_batched", p, dense)
        assert P.same_bits(dense, _launch_h2(p, row_last=[3, 9, 5], row_step=3)[0]), "row_last >= row_step everywhere must change nothing"
        out = _h2_out(p)
        for row_last in ([5, 1, 7], [0, 0, 0], [2, 3, 2]):
            dead = [i for i, r in enumerate(row_last) if r < 3]
            Xp = p.Xp.copy()
            x = Xp[:-32].reshape(3, -1)
            x[dead] = R.F16_NAN
            flat, _ = _launch_h2(p, Xp=Xp, row_last=row_last, row_step=3)
            _dead_items(out, flat, dense, dead, p.out0 if case.beta else None, (case.name, row_last))


# ---- row-sparse data gradient ---------------------------------------------------------------------------------------------------
def _sparse_cases():
    cs = []
    for Ho in (4, 8):
        for N in (3, 5, 64, 65):
            cs.append((f"halo-Ho{Ho}-N{N}", R._hc(f"sparse-halo-Ho{Ho}-N{N}", N, Ho, 64, 32, 32, 3, 1, 1, 1, 1, bias=False, ldc_pad=4 if Ho == 4 else 3)))
    cs.append(("cbm-8x32-N5", R._hc("sparse-cbm-8x32-N5", 5, 8, 32, 32, 132, 3, 1, 1, 1, 1, bias=False, ldc_pad=4)))
    cs.append(("tap-major-1x1-N5", R._hc("sparse-1x1-N5", 5, 4, 64, 64, 32, 1, 1, 0, 1, 1, bias=False)))
    cs.append(("dense-tiles-cross-images-N5", R._hc("sparse-not-6x64-N5", 5, 6, 64, 32, 32, 3, 1, 1, 1, 1, bias=False)))
    return cs


@pytest.mark.parametrize("name,case", _sparse_cases(), ids=[c[0] for c in _sparse_cases()])
def test_row_sparse_data_gradient_equals_dense_on_zeroed_rows(name, case):
    """mode 1 with row_last: live set none / all / mixed, beta 0 and 1, in the live-first order (N <= 64) and the plain one (N = 65): the launch on
    operands whose dead samples hold NaN planes equals, bit for bit, the dense launch on planes zeroed there; dead samples under beta 1 keep what
    they held.  Where tiles cross images (Ho Wo % 256 != 0) the call is dense: the result is the dense launch's."""
    N, PP = case.N_img, case.Ho * case.Wo
    g = np.random.Generator(np.random.PCG64(P.seed_of(name)))
    mixed = [int(v) for v in g.integers(0, 6, N)]
    mixed[0], mixed[-1] = 5, 0
    tiled = PP % 256 == 0
    for beta in (0, 1):
        c = case._replace(beta=beta)
        for kind in ("gauss", "lattice"):
            p = _h2(c, kind) if N <= 5 else _light_h2(c, kind)
            out = _h2_out(p)
            for row_last in ([0] * N, [5] * N, mixed):
                dead = [i for i, r in enumerate(row_last) if r < 3]
                rows = p.Xp[:-32].reshape(N, -1)
                zeroed, poisoned = p.Xp.copy(), p.Xp.copy()
                zeroed[:-32].reshape(N, -1)[dead] = 0
                if tiled:
                    poisoned[:-32].reshape(N, -1)[dead] = R.F16_NAN
                else:
                    poisoned = zeroed
                assert rows.shape[1] == case.Hi * case.Wi * p.ldx * 2
                want, _ = _launch_h2(p, Xp=zeroed)
                got, _ = _launch_h2(p, Xp=poisoned, row_last=row_last, row_step=3)
                assert out.pads_untouched(got) and out.pads_untouched(want)
                a, b = out.live(got)[0].reshape(N, PP, -1), out.live(want)[0].reshape(N, PP, -1)
                assert torch.isfinite(a).all(), (name, beta, kind, "a dead sample's operand rows were read")
                assert torch.equal(a, b), (name, beta, kind, row_last)
                live = [i for i in range(N) if i not in dead]
                assert P.same_bits(a[live], b[live]), (name, beta, kind, row_last)
                if beta and tiled:
                    assert P.same_bits(a[dead], p.out0[0].reshape(N, PP, -1)[dead])
                elif tiled:
                    assert (a[dead].view(torch.int32) == 0).all()


class _Light:
    pass


@functools.lru_cache(maxsize=None)
def _light_h2(c, kind):
    """operands of a many-sample case without its fp64 restatement (the comparison is between two launches)"""
    p = _Light()
    s = P.seed_of("light" + kind + c.name)
    p.c, p.kind, p.K, p.M, p.xrows = c, kind, c.KH * c.KW * c.Kc, c.N_img * c.Ho * c.Wo, c.N_img * c.Hi * c.Wi
    p.ldx, p.ldc = c.Kc + c.ldx_pad, c.Nout + c.ldc_pad
    x, w = R.make(kind, (1, p.xrows, c.Kc), (), s), R.make(kind, (1, c.Nout, p.K), (), s + 1)
    p.sx, p.sw = R.scale_of(np.abs(x).max()), np.full(1, R.scale_of(np.abs(w).max()), np.float32)
    x1, x2 = R.split2(x, p.sx)
    w1, w2 = R.split2(w, p.sw[0])
    p.Xp, p.Wp = R.pack(x1[0], x2[0], p.ldx), R.pack(w1[0], w2[0])
    unit = abs(c.alpha) * 4096.0 / (float(p.sx) * float(p.sw[0]))
    g = np.random.Generator(np.random.PCG64(s + 2))
    p.bias = None
    p.out0 = torch.from_numpy((g.integers(-8, 9, (1, p.M, c.Nout)) * unit).astype(np.float32)) if c.beta else None
    return p


# ====================================================================================================================
# sp_conv_wgrad_f16x2 / _f16x1
# ====================================================================================================================
def _hw_out(p):
    return P.Guarded(p.c.nbatch, p.c.Co, p.Nvalid, p.ldo, p.c.Co * p.ldo, fill="sentinel", data=None if p.out0 is None else p.out0[..., :p.Nvalid])


def _launch_hw(p, *, Yp=None, row_last=None, row_step=0, null=(), off=None, desc=None, expect=0):
    hip, L = P.abi()
    c = p.c
    off = off or {}
    dX, dY, dsx, dsy = P.u16(p.Xp), P.u16(p.Yp if Yp is None else Yp), P.f32(p.sx), P.f32(p.sy)
    out = _hw_out(p)
    dO = P.up(out)
    drl = None if row_last is None else torch.tensor(row_last, dtype=torch.int32, device=P.dev())
    d = R.hw_desc(hip, p, row_last=None if drl is None else drl.data_ptr(), row_step=row_step, **(desc or {}))
    nbytes = L.sp_conv_wgrad_f16x2_workspace(ctypes.byref(d))
    if expect == 0:
        assert nbytes == (p.splits * c.Co * p.ldo * 4 if p.splits > 1 else 0), (c.name, nbytes, p.splits)
    dWs = P.output(nbytes // 4) if nbytes else None          # exactly the queried size between sentinels
    ptr = {"X": dX.data_ptr() + off.get("X", 0), "Y": dY.data_ptr() + off.get("Y", 0), "sx": dsx.data_ptr(), "sy": dsy.data_ptr(), "out": P.at(dO),
           "ws": P.at(dWs)}
    for k in null:
        ptr[k] = None
    fn = L.sp_conv_wgrad_f16x2 if c.nprod == 3 else L.sp_conv_wgrad_f16x1
    rc = fn(ctypes.byref(d), ptr["X"], ptr["sx"], ptr["Y"], ptr["sy"], ptr["out"], ptr["ws"], hip.stream())
    torch.cuda.synchronize()
    assert rc == expect, (c.name, rc, expect)
    flat = dO.flat()
    if dWs is not None:
        assert dWs.pads_untouched(), f"{c.name}: a word around the slab workspace changed"
        assert expect == 0 or dWs.untouched()
    if expect != 0:
        assert out.all_untouched(flat), f"{c.name}: a refused call wrote to the output"
    return flat


def _check_hw(group, p, flat):
    _check(group, p, _hw_out(p), flat, f"{p.c.name} [{p.kind}] {p.build} (splits {p.splits})", 3e-6, slice(p.Nvalid))


def _run_hw(group, case, kinds=("gauss", "lattice")):
    for kind in kinds:
        p = _hw(case, kind)
        flat = _launch_hw(p)
        _check_hw(group, p, flat)
        if p.splits > 1:
            assert P.same_bits(flat, _launch_hw(p)), f"{case.name}: two slab launches differ"


@pytest.mark.parametrize("case", R.hw_cases(), ids=lambda c: c.name)
def test_wgrad(case):
    _run_hw("f16x2_wgrad", case, ("gauss", "lattice", "heavy") if case.name.startswith("rows") or "conv-3x3-slabs" in case.name else ("gauss", "lattice"))


@pytest.mark.parametrize("case", R.hw_x1_cases(), ids=lambda c: c.name)
def test_wgrad_one_product(case):
    _run_hw("f16x1_wgrad", case)


@pytest.mark.parametrize("case", R.hw_batched_cases(), ids=lambda c: c.name)
def test_wgrad_batched_and_dead_items(case):
    """nbatch 3 (one TN GEMM per item, no workspace), Ci padded to 16 with ldo 12 (< Ci: only Nvalid = 12 columns exist) and 20; with row_last
    the live items equal the dense launch bit for bit, dead items (NaN gradient planes: not read) are zeros under beta 0, left alone under beta 1"""
    for kind in ("gauss", "lattice"):
        p = _hw(case, kind)
        dense = _launch_hw(p)
        _check_hw("f16x2_wgrad_batched", p, dense)
        out = _hw_out(p)
        for row_last in ([5, 1, 7], [0, 0, 0], [3, 3, 3]):
            dead = [i for i, r in enumerate(row_last) if r < 3]
            Yp = p.Yp.copy()
            Yp[:-32].reshape(3, -1)[dead] = R.F16_NAN
            flat = _launch_hw(p, Yp=Yp, row_last=row_last, row_step=3)
            _dead_items(out, flat, dense, dead, p.out0[..., :p.Nvalid] if case.beta else None, (case.name, row_last))


# ====================================================================================================================
# sp_conv_wgrad_f16x2_multi (hw2_kernel)
# ====================================================================================================================
# (name, N, H, W, k, nseg, per-application gradient scales (cycled), row_last, seg_steps, beta, kinds)
MULTI = [("1x1-nseg1", 1, 32, 64, 1, 1, (1.0,), None, None, 0, ("gauss", "lattice")),
         ("1x1-nseg3-scales", 1, 32, 64, 1, 3, (1.0, 2.0 ** -20, 2.0 ** 8), None, None, 1, ("gauss",)),
         ("1x1-nseg3-lattice", 1, 32, 64, 1, 3, (1.0, 0.5, 4.0), None, None, 1, ("lattice",)),
         ("1x1-nseg16", 1, 32, 64, 1, 16, (1.0, 2.0 ** -20, 2.0 ** 8), None, None, 0, ("gauss",)),
         ("3x3-nseg3", 1, 32, 64, 3, 3, (1.0, 2.0, 0.25), None, None, 0, ("gauss", "lattice")),
         ("1x1-nseg3-row-last", 2, 16, 64, 1, 3, (1.0, 2.0, 0.5), [1, 3], [1, 2, 4], 1, ("gauss", "lattice")),       # sample 0 skipped in two, all in one
         ("3x3-nseg3-row-last", 4, 8, 64, 3, 3, (1.0,), [2, 0, 3, 1], [1, 2, 3], 0, ("gauss", "lattice"))]


@pytest.mark.parametrize("row", MULTI, ids=[r[0] for r in MULTI])
def test_wgrad_multi(row):
    """dW = alpha sum_g dY_g^T X_g (+ dW) in ONE launch, against the sum of the per-application references, every application with its own scales;
    pixels of samples with row_last[img] < seg_steps[g] hold NaN planes and are skipped; slabs twice bit-identical; on lattice data exact"""
    name, N, H, W, k, nseg, muls, row_last, seg_steps, beta, kinds = row
    hip, L = P.abi()
    Ci = Co = 256
    base = R._wc("multi-" + name, N, H, W, Ci, Co, k, 1, k // 2, 1, alpha=-0.5, beta=0, ldo_pad=4, ldy_pad=16)
    PP = H * W
    for kind in kinds:
        ps = []
        for g in range(nseg):
            dead = None
            if row_last is not None:
                dead = np.concatenate([np.arange(b * PP, (b + 1) * PP) for b in range(N) if row_last[b] < seg_steps[g]] + [np.zeros(0, np.int64)])
            # (lattice: a quarter of the entries non-zero and q = 0, so that the SUM over the applications, in units of the smallest
            # application's lattice, still meets the exactness condition asserted below)
            ps.append(R.HWProblem(base, kind, seed_extra=f"seg{g}", dy_mul=muls[g % len(muls)], dead_rows=dead, **(dict(keep=0.25, qmax=1) if kind == "lattice" else {})))
        p0 = ps[0]
        M, Ntot, ldo = p0.M, p0.Ntot, p0.ldo
        assert R.hw2_applies(base, nseg, ldo)
        splits = R.hw2_splits(M, Co, Ntot, nseg)
        d = R.hw_desc(hip, p0, beta=beta)
        nbytes = L.sp_conv_wgrad_f16x2_multi_workspace(ctypes.byref(d), nseg)
        assert nbytes == nseg * splits * Co * ldo * 4, (nbytes, splits)
        ref = sum(p.planes()[0] for p in ps)
        S = sum(p.planes()[1] for p in ps)
        unit = min(p.unit.min() for p in ps)
        g = np.random.Generator(np.random.PCG64(P.seed_of(name + kind)))
        out0 = None
        if beta:
            out0 = torch.from_numpy((g.integers(-8, 9, (1, Co, Ntot)) * (unit if kind == "lattice" else 1.0)).astype(np.float32))
            ref, S = ref + out0.double(), S + out0.double().abs()
        out = P.Guarded(1, Co, Ntot, ldo, fill="sentinel", data=out0)
        keep = [(P.u16(p.Xp), P.u16(p.Yp), P.f32(p.sx), P.f32(p.sy)) for p in ps]
        arr = lambda i: (ctypes.c_void_p * nseg)(*[t[i].data_ptr() for t in keep])
        drl = None if row_last is None else torch.tensor(row_last, dtype=torch.int32, device=P.dev())
        steps = None if seg_steps is None else (ctypes.c_int * nseg)(*seg_steps)

        def launch():
            dO, dWs = P.up(out), P.output(nbytes // 4)
            rc = L.sp_conv_wgrad_f16x2_multi(ctypes.byref(d), nseg, arr(0), arr(2), arr(1), arr(3), P.at(dO), P.at(dWs),
                                             None if drl is None else drl.data_ptr(), None if steps is None else ctypes.addressof(steps), hip.stream())
            torch.cuda.synchronize()
            assert rc == 0, (name, rc)
            assert dWs.pads_untouched(), f"{name}: a word around the slab workspace changed"
            return dO.flat()
        flat = launch()
        chain = R.chain_hw2(M, splits, nseg)
        SUM.judge("f16x2_wgrad_multi", f"{name} [{kind}] hw2+hw_reduce4 (splits {splits})", out, flat, ref, S, chain, 3e-6)
        true = sum(p.true() for p in ps) + (0 if out0 is None else out0.double())
        P.close(out.live(flat), true, 3e-6, name)
        assert P.same_bits(flat, launch()), f"{name}: two launches differ"
        if kind == "lattice":
            assert float((S / unit).max()) <= 2.0 ** 24
            assert torch.equal(out.live(flat).double(), ref), f"{name}: not the exact result"


# ====================================================================================================================
# refusals: one row per `return SP_EINVAL` / `SP_ENULL` of the entry points
# ====================================================================================================================
_G = R._hg("refusal-gemm", 256, 32, 64, 0, ldx_pad=0, ldc_pad=0)
_B = R._hg("refusal-batched", 256, 32, 64, 0, nbatch=2, ldx_pad=0, ldc_pad=0)
_S = R._hc("refusal-stats", 1, 16, 16, 32, 64, 3, 1, 1, 1, 0, bias=False, stats=True, ldc_pad=0, alpha=1.0)
H2_REFUSALS = [
    ("X-null", _G, dict(null=("X",)), ENULL), ("W-null", _G, dict(null=("W",)), ENULL), ("x_scale-null", _G, dict(null=("sx",)), ENULL),
    ("w_scale-null", _G, dict(null=("sw",)), ENULL), ("out-null", _G, dict(null=("out",)), ENULL),
    ("mode2", _G, dict(desc=dict(mode=2)), EINVAL), ("Kc%32", _G, dict(desc=dict(Kc=48, ldx=48)), EINVAL), ("ldx<Kc", _G, dict(desc=dict(ldx=16)), EINVAL),
    ("ldx%16", _G, dict(desc=dict(ldx=40)), EINVAL), ("X+8B", _G, dict(off=dict(X=8)), EINVAL), ("W+8B", _G, dict(off=dict(W=8)), EINVAL),
    ("nbatch0", _G, dict(desc=dict(nbatch=0)), EINVAL), ("stride0", _G, dict(desc=dict(stride=0)), EINVAL), ("dil0", _G, dict(desc=dict(dil=0)), EINVAL),
    ("Nout0", _G, dict(desc=dict(Nout=0)), EINVAL), ("M0", _G, dict(desc=dict(N_img=0)), EINVAL),
    ("batched-mode1", _B, dict(desc=dict(mode=1)), EINVAL), ("batched-3x3", _B, dict(desc=dict(KH=3, KW=3)), EINVAL),
    ("batched-stride2", _B, dict(desc=dict(stride=2)), EINVAL), ("batched-pad1", _B, dict(desc=dict(pad=1)), EINVAL),
    ("batched-rows%256", _B, dict(desc=dict(N_img=255, strideX=255 * 32, strideC=255 * 64)), EINVAL),
    ("batched-strideX", _B, dict(desc=dict(strideX=256 * 32 + 16)), EINVAL), ("batched-strideC", _B, dict(desc=dict(strideC=256 * 64 + 4)), EINVAL),
    ("batched-strideW", _B, dict(desc=dict(strideW=0)), EINVAL), ("batched-one-product", _B._replace(nprod=1), {}, EINVAL),
    ("batched-stats", _B._replace(stats=True, bias=False), {}, EINVAL),
    ("stats-beta", _S, dict(desc=dict(beta=1)), EINVAL), ("stats-relu", _S, dict(desc=dict(relu=1)), EINVAL), ("stats-mode1", _S, dict(desc=dict(mode=1)), EINVAL),
    ("stats-st_partial-null", _S, dict(null=("stp",)), ENULL), ("stats-st_mm-null", _S, dict(null=("stm",)), ENULL),
]


@pytest.mark.parametrize("name,case,how,rc", H2_REFUSALS, ids=[r[0] for r in H2_REFUSALS])
def test_igemm_refusals(name, case, how, rc):
    """the code the header states, before anything is launched: the output (and the statistics) stay all-sentinel"""
    _launch_h2(_h2(case, "gauss"), expect=rc, **how)


_W = R._wg("refusal-wgrad", 64, 32, 32, ldy_pad=0, ldo_pad=0)
_WS = R._wg("refusal-wgrad-slabs", 2049, 48, 32)
_WB = R._wg("refusal-wgrad-batched", 32, 32, 16, nbatch=2, ldy_pad=0, ldo_pad=0)
HW_REFUSALS = [
    ("X-null", _W, dict(null=("X",)), ENULL), ("dY-null", _W, dict(null=("Y",)), ENULL), ("x_scale-null", _W, dict(null=("sx",)), ENULL),
    ("y_scale-null", _W, dict(null=("sy",)), ENULL), ("dW-null", _W, dict(null=("out",)), ENULL),
    ("Ci%16", _W, dict(desc=dict(Ci=24, ldx=24)), EINVAL), ("Co%16", _W, dict(desc=dict(Co=24)), EINVAL), ("ldx!=Ci", _W, dict(desc=dict(ldx=48)), EINVAL),
    ("ldy<Co", _W, dict(desc=dict(ldy=16)), EINVAL), ("ldy%16", _W, dict(desc=dict(ldy=40)), EINVAL), ("nbatch0", _W, dict(desc=dict(nbatch=0)), EINVAL),
    ("X+8B", _W, dict(off=dict(X=8)), EINVAL), ("dY+8B", _W, dict(off=dict(Y=8)), EINVAL), ("ldo<Ntot", _W, dict(desc=dict(ldo=28)), EINVAL),
    ("M0", _W, dict(desc=dict(N_img=0)), EINVAL), ("slabs-workspace-null", _WS, dict(null=("ws",)), ENULL),
    ("batched-3x3", _WB, dict(desc=dict(KH=3, KW=3)), EINVAL), ("batched-stride2", _WB, dict(desc=dict(stride=2)), EINVAL),
    ("batched-pad1", _WB, dict(desc=dict(pad=1)), EINVAL), ("batched-rows%32", _WB, dict(desc=dict(N_img=31, strideX=31 * 16, strideY=31 * 32)), EINVAL),
    ("batched-strideX", _WB, dict(desc=dict(strideX=32 * 16 + 16)), EINVAL), ("batched-strideY", _WB, dict(desc=dict(strideY=0)), EINVAL),
    ("batched-strideO", _WB, dict(desc=dict(strideO=32 * 16 + 4)), EINVAL), ("batched-x_scale_vec", _WB, dict(desc=dict(x_scale_vec=1)), EINVAL),
    ("batched-y_scale_vec", _WB, dict(desc=dict(y_scale_vec=1)), EINVAL), ("batched-one-product", _WB._replace(nprod=1), {}, EINVAL),
]


@pytest.mark.parametrize("name,case,how,rc", HW_REFUSALS, ids=[r[0] for r in HW_REFUSALS])
def test_wgrad_refusals(name, case, how, rc):
    _launch_hw(_hw(case, "gauss"), expect=rc, **how)


MULTI_REFUSALS = [("Xsplits-null", dict(null=0), ENULL), ("x_scales-null", dict(null=1), ENULL), ("dYsplits-null", dict(null=2), ENULL),
                  ("y_scales-null", dict(null=3), ENULL), ("dW-null", dict(null=4), ENULL), ("workspace-null", dict(null=5), ENULL),
                  ("nseg0", dict(nseg=0), EINVAL), ("nseg17", dict(nseg=17), EINVAL), ("Wo20", dict(desc=dict(Wi=20, Wo=20)), EINVAL),
                  ("Co128", dict(desc=dict(Co=128)), EINVAL), ("rows2016", dict(desc=dict(Hi=63, Ho=63, Wi=32, Wo=32)), EINVAL),
                  ("ldo%4", dict(desc=dict(ldo=258)), EINVAL), ("stride2", dict(desc=dict(stride=2)), EINVAL), ("nbatch2", dict(desc=dict(nbatch=2)), EINVAL),
                  ("row_last-without-seg_steps", dict(row_last=True), ENULL), ("seg_steps-without-row_last", dict(seg_steps=True), ENULL),
                  ("an-X-null", dict(inner=(0, None)), ENULL), ("a-y_scale-null", dict(inner=(3, None)), ENULL), ("a-dY+8B", dict(inner=(2, 8)), EINVAL)]


@pytest.mark.parametrize("name,how,rc", MULTI_REFUSALS, ids=[r[0] for r in MULTI_REFUSALS])
def test_wgrad_multi_refusals(name, how, rc):
    """the workspace query returns 0 where the shape constraints do not hold, and the launch its code; dW and the workspace stay all-sentinel"""
    hip, L = P.abi()
    nseg = how.get("nseg", 2)
    n = max(1, min(nseg, 16))
    a = dict(N_img=1, Hi=32, Wi=64, Ci=256, ldx=256, Ho=32, Wo=64, Co=256, ldy=256, KH=1, KW=1, stride=1, pad=0, dil=1, ldo=256, beta=0, alpha=1.0, nbatch=1)
    a.update(how.get("desc", {}))
    d = hip.WgradDesc(**a)
    if "desc" in how or "nseg" in how:
        assert L.sp_conv_wgrad_f16x2_multi_workspace(ctypes.byref(d), nseg) == 0
    planes = torch.zeros(2048 * 256 * 2 + 32, dtype=torch.int16, device=P.dev())
    one = P.f32([1.0])
    dO, dWs = P.up(P.Guarded(1, 256, 256, 260, fill="sentinel")), P.output(4096)
    cols = [[planes.data_ptr()] * n, [one.data_ptr()] * n, [planes.data_ptr()] * n, [one.data_ptr()] * n]
    if "inner" in how:
        i, v = how["inner"]
        cols[i][n - 1] = None if v is None else cols[i][n - 1] + v
    args = [(ctypes.c_void_p * n)(*col) for col in cols] + [P.at(dO), P.at(dWs)]
    if "null" in how:
        args[how["null"]] = None
    drl = torch.zeros(1, dtype=torch.int32, device=P.dev())
    steps = (ctypes.c_int * n)(*([0] * n))
    rc_got = L.sp_conv_wgrad_f16x2_multi(ctypes.byref(d), nseg, *args, drl.data_ptr() if how.get("row_last") else None,
                                         ctypes.addressof(steps) if how.get("seg_steps") else None, hip.stream())
    torch.cuda.synchronize()
    assert rc_got == rc, (name, rc_got)
    assert dO.untouched() and dWs.untouched(), f"{name}: a refused call wrote"


SPLIT_REFUSALS = [
    ("split2-x-null", "sp_split2_f16", lambda x, o, s: (None, 32, o, s, 0), ENULL), ("split2-out-null", "sp_split2_f16", lambda x, o, s: (x, 32, None, s, 0), ENULL),
    ("split2-scale-null", "sp_split2_f16", lambda x, o, s: (x, 32, o, None, 0), ENULL), ("split2-n%16", "sp_split2_f16", lambda x, o, s: (x, 40, o, s, 0), EINVAL),
    ("wT-w-null", "sp_split2_f16_wT", lambda x, o, s: (None, 16, 1, 4, o, s), ENULL), ("wT-out-null", "sp_split2_f16_wT", lambda x, o, s: (x, 16, 1, 4, None, s), ENULL),
    ("wT-scale-null", "sp_split2_f16_wT", lambda x, o, s: (x, 16, 1, 4, o, None), ENULL), ("wT-tapsCo%16", "sp_split2_f16_wT", lambda x, o, s: (x, 8, 3, 4, o, s), EINVAL),
    ("rows-w-null", "sp_split2_f16_rows", lambda x, o, s: (None, 2, 32, 16, None, o, s), ENULL),
    ("rows-out-null", "sp_split2_f16_rows", lambda x, o, s: (x, 2, 32, 16, None, None, s), ENULL),
    ("rows-scale-null", "sp_split2_f16_rows", lambda x, o, s: (x, 2, 32, 16, None, o, None), ENULL),
    ("rows-rows0", "sp_split2_f16_rows", lambda x, o, s: (x, 0, 32, 16, None, o, s), EINVAL), ("rows-K8", "sp_split2_f16_rows", lambda x, o, s: (x, 2, 8, 8, None, o, s), EINVAL),
    ("rows-K%16", "sp_split2_f16_rows", lambda x, o, s: (x, 2, 40, 8, None, o, s), EINVAL),
    ("rows-absorb-Kc2", "sp_split2_f16_rows", lambda x, o, s: (x, 2, 32, 2, x, o, s), EINVAL),
    ("rows-absorb-Kc%4", "sp_split2_f16_rows", lambda x, o, s: (x, 2, 36 * 4, 6, x, o, s), EINVAL),
    ("rows-absorb-K%Kc", "sp_split2_f16_rows", lambda x, o, s: (x, 2, 32, 12, x, o, s), EINVAL),
    ("rows-w+4B", "sp_split2_f16_rows", lambda x, o, s: (x + 4, 2, 32, 16, None, o, s), EINVAL),
    ("rows-absorb+4B", "sp_split2_f16_rows", lambda x, o, s: (x, 2, 32, 16, x + 4, o, s), EINVAL),
    ("wT_rows-w-null", "sp_split2_f16_wT_rows", lambda x, o, s: (None, 1, 16, 1, 4, None, o, s), ENULL),
    ("wT_rows-out-null", "sp_split2_f16_wT_rows", lambda x, o, s: (x, 1, 16, 1, 4, None, None, s), ENULL),
    ("wT_rows-scale-null", "sp_split2_f16_wT_rows", lambda x, o, s: (x, 1, 16, 1, 4, None, o, None), ENULL),
    ("wT_rows-nbatch0", "sp_split2_f16_wT_rows", lambda x, o, s: (x, 0, 16, 1, 4, None, o, s), EINVAL),
    ("wT_rows-nbatch65536", "sp_split2_f16_wT_rows", lambda x, o, s: (x, 65536, 16, 1, 4, None, o, s), EINVAL),
    ("wT_rows-tapsCo%16", "sp_split2_f16_wT_rows", lambda x, o, s: (x, 1, 8, 3, 4, None, o, s), EINVAL),
    ("wT_rows-Ci%4", "sp_split2_f16_wT_rows", lambda x, o, s: (x, 1, 16, 1, 6, None, o, s), EINVAL),
    ("wT_rows-Ci2", "sp_split2_f16_wT_rows", lambda x, o, s: (x, 1, 16, 1, 2, None, o, s), EINVAL),
    ("wT_rows-w+4B", "sp_split2_f16_wT_rows", lambda x, o, s: (x + 4, 1, 16, 1, 4, None, o, s), EINVAL),
    ("cols-x-null", "sp_split2_f16_cols", lambda x, o, s: (None, 2, 16, o, s, x), ENULL), ("cols-out-null", "sp_split2_f16_cols", lambda x, o, s: (x, 2, 16, None, s, x), ENULL),
    ("cols-scale-null", "sp_split2_f16_cols", lambda x, o, s: (x, 2, 16, o, None, x), ENULL), ("cols-scratch-null", "sp_split2_f16_cols", lambda x, o, s: (x, 2, 16, o, s, None), ENULL),
    ("cols-rows0", "sp_split2_f16_cols", lambda x, o, s: (x, 0, 16, o, s, x), EINVAL), ("cols-C8", "sp_split2_f16_cols", lambda x, o, s: (x, 2, 8, o, s, x), EINVAL),
    ("cols-C%16", "sp_split2_f16_cols", lambda x, o, s: (x, 2, 24, o, s, x), EINVAL), ("cols-x+4B", "sp_split2_f16_cols", lambda x, o, s: (x + 4, 2, 16, o, s, x), EINVAL),
    ("cols-col_scale+4B", "sp_split2_f16_cols", lambda x, o, s: (x, 2, 16, o, s + 4, x), EINVAL),
    ("cols-scratch+4B", "sp_split2_f16_cols", lambda x, o, s: (x, 2, 16, o, s, x + 4), EINVAL),
]


@pytest.mark.parametrize("name,fn,args,rc", SPLIT_REFUSALS, ids=[r[0] for r in SPLIT_REFUSALS])
def test_splitter_refusals(name, fn, args, rc):
    hip, L = P.abi()
    x, out, sc = P.raw(4096 * 4, init=np.ones(4096, np.float32)), P.raw(4096 * 4), P.raw(256)
    assert getattr(L, fn)(*args(x.ptr, out.ptr, sc.ptr), hip.stream()) == rc, name
    torch.cuda.synchronize()
    assert out.untouched() and sc.untouched() and x.untouched(), f"{name}: a refused call wrote"
    if fn == "sp_split2_f16_cols" and rc == EINVAL and "+4B" not in name:
        a = args(x.ptr, out.ptr, sc.ptr)
        assert L.sp_split2_f16_cols_workspace(a[1], a[2]) == 0
