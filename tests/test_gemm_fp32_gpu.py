"""The three fp32 GEMM kernels through the C ABI -- sp_conv_igemm (forward, data gradient, batched GEMM, split-K), sp_gemm_skinny and sp_conv_wgrad --
against the plain fp64 restatement of tests/gemm_ref.py (held to torch's fp64 conv and autograd by tests/test_gemm_ref_cpu.py), at the tile, chunk,
slice and split edges listed there.

Every operand and output lies inside a larger allocation (parity.Guarded): operand pads, batch gaps and guards are NaN, output pads, gaps, guards
and workspace tails a sentinel word.  After each launch every sentinel word must be unchanged and every live word finite and inside the ELEMENT-WISE
bar |got - ref| <= c 2^-24 S + 2^-149 (S the contraction over absolute values, c the launch's longest chain of dependent roundings, derived in
gemm_ref.py).  The max-norm bars of tests/test_ops_gpu.py (3e-6 sqrt(K / 32) for GEMMs, 2e-6 / 3e-6 for convs, against max(1, max|ref|)) stay as a
second, weaker assertion.  Launches on a split path run twice and must be bit-identical.  Each case prints its err / bar; the module prints one
summary line per group at its end (profiles/gemm_fp32_parity.md)."""
import ctypes
import functools
import math

import pytest
import torch

import gemm_ref as R
import parity as P

pytestmark = pytest.mark.gpu

SUM = P.Summary()
_summary = SUM.fixture()
# the operands and the fp64 restatement of a case, built once
_igemm_problem, _skinny_problem, _wgrad_problem = (functools.lru_cache(maxsize=None)(cls) for cls in (R.IgemmProblem, R.SkinnyProblem, R.WgradProblem))


def _gemm_legacy(K):
    return 3e-6 * math.sqrt(max(K, 32) / 32)


# ====================================================================================================================
# launches
# ====================================================================================================================
def _igemm_desc(hip, p, ws_ptr=None, ksplit=0):
    c = p.c
    return hip.ConvDesc(N_img=c.N_img, Hi=c.Hi, Wi=c.Wi, Kc=c.Kc, ldx=p.ldx, Ho=c.Ho, Wo=c.Wo, Nout=c.Nout, ldc=p.ldc, KH=c.KH, KW=c.KW,
                        stride=c.stride, pad=c.pad, dil=c.dil, mode=c.mode, ldw=p.ldw, alpha=c.alpha, beta=c.beta, relu=int(c.relu), nbatch=c.nbatch,
                        strideX=p.sX, strideW=p.sW, strideC=p.sC, ksplit=ksplit, workspace=ws_ptr)


def _launch_igemm(p, ksplit):
    """one sp_conv_igemm launch on fresh copies of the guarded buffers -> (output allocation, workspace allocation or None), on the host"""
    hip, L = P.abi()
    dX, dW, dO = P.up(p.X), P.up(p.W), P.up(p.out)
    dB, dWs = P.operand(p.bias), P.up(p.ws if ksplit > 1 else None)
    d = _igemm_desc(hip, p, P.at(dWs), ksplit)
    rc = L.sp_conv_igemm(ctypes.byref(d), P.at(dX), P.at(dW), P.at(dB), P.at(dO), hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, (p.c.name, rc)
    return dO.flat(), (None if dWs is None else dWs.flat())


def _run_igemm(group, p, legacy):
    c = p.c
    ref, S = p.reference()
    flat, ws_after = _launch_igemm(p, c.ksplit)
    SUM.judge(group, c.name, p.out, flat, ref, S, p.chain, legacy)
    if c.ksplit > 1:
        assert p.ws.pads_untouched(ws_after), f"{c.name}: a word around the split-K workspace changed"
        split = R.igemm_plan(c.Kc, c.KH * c.KW, c.ksplit, c.nbatch, c.mode)[2] > 1
        if split:
            again, _ = _launch_igemm(p, c.ksplit)
            assert P.same_bits(flat, again), f"{c.name}: two split-K launches differ"
            live = p.ws.live(ws_after).reshape(c.ksplit, -1)
            used = R.igemm_plan(c.Kc, 1, c.ksplit)[2]
            assert torch.isfinite(live[:used]).all() and p.ws.live(ws_after.view(torch.int32)).reshape(c.ksplit, -1)[used:].eq(P.SENTINEL).all(), \
                f"{c.name}: the slabs in use are {used} of {c.ksplit}"
        else:            # ksplit is not honoured (batched, or more than one tap): the unsplit result, and the workspace is never touched
            assert p.ws.all_untouched(ws_after), f"{c.name}: the workspace of an ignored ksplit was written"
            plain, _ = _launch_igemm(p, 0)
            assert P.same_bits(flat, plain), f"{c.name}: an ignored ksplit changed the result"
    return flat


@pytest.mark.parametrize("case", R.igemm_gemm_cases(), ids=lambda c: c.name)
def test_igemm_as_gemm(case):
    _run_igemm("igemm_gemm", _igemm_problem(case), _gemm_legacy(case.Kc))


@pytest.mark.parametrize("case", R.igemm_conv_cases(), ids=lambda c: c.name)
def test_igemm_as_conv(case):
    _run_igemm("igemm_conv", _igemm_problem(case), 2e-6)


def _launch_skinny(p, *, offs=None, null=()):
    """one sp_gemm_skinny launch -> (rc, output allocation on the host).  offs: byte offsets added to A, B, C, bias, workspace; null: names passed as
    NULL"""
    hip, L = P.abi()
    c = p.c
    offs = offs or {}
    dA, dB, dO = P.up(p.A_buf), P.up(p.B_buf), P.up(p.out)
    dBias = P.operand(p.bias)
    nbytes = L.sp_gemm_skinny_workspace(c.M, c.N, c.K, c.layout)
    dWs = P.output(nbytes // 4) if nbytes else None
    ptrs = {"A": P.at(dA, offs.get("A", 0)), "B": P.at(dB, offs.get("B", 0)), "C": P.at(dO, offs.get("C", 0)),
            "bias": P.at(dBias, offs.get("bias", 0)), "ws": P.at(dWs, offs.get("ws", 0))}
    for k in null:
        ptrs[k] = None
    rc = L.sp_gemm_skinny(ptrs["A"], ptrs["B"], ptrs["bias"], ptrs["C"], c.M, c.N, c.K, p.lda, p.ldb, p.ldc, c.layout, c.alpha, int(c.relu),
                          ptrs["ws"], hip.stream())
    torch.cuda.synchronize()
    if dWs is not None:
        assert dWs.pads_untouched(), f"{c.name}: a word around the slice workspace changed"
    return rc, dO.flat()


@pytest.mark.parametrize("case", R.skinny_cases(), ids=lambda c: c.name)
def test_skinny(case):
    """sp_gemm_skinny, and -- sp_gemm_skinny_applies holds for every case -- sp_conv_igemm on the same guarded operands: both inside the bar (each
    with its own chain); bit equality between the two kernels is not asked"""
    hip, L = P.abi()
    p, c = _skinny_problem(case), case
    assert L.sp_gemm_skinny_applies(c.M, c.N, c.K, p.lda, p.ldb, p.ldc, c.layout) == 1
    ref, S = p.reference()
    rc, flat = _launch_skinny(p)
    assert rc == 0, rc
    SUM.judge("skinny", c.name, p.out, flat, ref, S, p.chain, _gemm_legacy(c.K))
    if p.nsplit > 1:
        rc, again = _launch_skinny(p)
        assert rc == 0 and P.same_bits(flat, again), f"{c.name}: two sliced launches differ"
    # the same operands through the 128-row tile kernel
    dA, dB, dO = P.up(p.A_buf), P.up(p.B_buf), P.up(p.out)
    dBias = P.operand(p.bias)
    d = hip.ConvDesc(N_img=c.M, Hi=1, Wi=1, Kc=c.K, ldx=p.lda, Ho=1, Wo=1, Nout=c.N, ldc=p.ldc, KH=1, KW=1, stride=1, pad=0, dil=1, mode=c.layout,
                     ldw=p.ldb, alpha=c.alpha, beta=0, relu=int(c.relu), nbatch=1)
    rc = L.sp_conv_igemm(ctypes.byref(d), P.at(dA), P.at(dB), P.at(dBias), P.at(dO), hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    SUM.judge("skinny_vs_igemm", c.name, p.out, dO.flat(), ref, S, R.chain_igemm(c.K, 1), _gemm_legacy(c.K))


@pytest.mark.parametrize("r", R.skinny_refusals(), ids=lambda r: r.name)
def test_skinny_refusals(r):
    """every call outside the domain of include/scanpaths_amd.h returns its code before anything is launched: the output stays all-sentinel"""
    hip, L = P.abi()
    p = R.SkinnyProblem(R._SK(r.name, r.M, r.N, r.K, r.layout if r.layout in (0, 1) else 1, 1.0, True, False, r.ldc_pad, 0))
    p.lda, p.ldb = r.K + r.lda_pad, (r.K if r.layout == 0 else r.N) + r.ldb_pad
    p.c = p.c._replace(layout=r.layout)
    assert L.sp_gemm_skinny_applies(r.M, r.N, r.K, p.lda, p.ldb, p.ldc, r.layout) == r.applies
    offs = {k: v for k, v in (("A", r.offA), ("B", r.offB), ("C", r.offC), ("bias", r.offBias), ("ws", r.offWs))}
    null = tuple(k for k, v in offs.items() if v is None)
    rc, flat = _launch_skinny(p, offs={k: v for k, v in offs.items() if v}, null=null)
    assert rc == r.rc, (r, rc)
    assert p.out.all_untouched(flat), f"{r.name}: a refused call wrote to the output"


def _launch_wgrad(p):
    hip, L = P.abi()
    d = p.desc(hip)
    splits, nbytes = R.wgrad_splits(L, d, p.c.Co, p.ldo)
    dX, dY, dO = P.up(p.X), P.up(p.dY), P.up(p.out)
    dWs = P.output(nbytes // 4) if nbytes else None          # exactly the queried size, sentinels around it
    rc = L.sp_conv_wgrad(ctypes.byref(d), P.at(dX), P.at(dY), P.at(dO), P.at(dWs), hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, (p.c.name, rc)
    if dWs is not None:
        assert dWs.pads_untouched(), f"{p.c.name}: a word around the slab workspace changed"
    return splits, dO.flat()


def _run_wgrad(group, p, legacy):
    ref, S = p.reference()
    splits, flat = _launch_wgrad(p)
    SUM.judge(group, p.c.name + f" (splits {splits})", p.out, flat, ref, S, R.chain_wgrad(p.M, splits), legacy)
    if splits > 1:
        assert P.same_bits(flat, _launch_wgrad(p)[1]), f"{p.c.name}: two slab launches differ"
    return flat


@pytest.mark.parametrize("case", R.wgrad_cases(), ids=lambda c: c.name)
def test_wgrad(case):
    p = _wgrad_problem(case)
    _run_wgrad("wgrad", p, _gemm_legacy(p.M) if case.KH == 1 else 3e-6)


# ====================================================================================================================
# the dispatcher: functional._igemm through functional.gemm
# ====================================================================================================================
# (name, M, K, N, layout, bias off by one float)
DISPATCH = [("skinny-forward-and-dgrad", 64, 64, 64, "nk", False), ("skinny-kn", 33, 128, 64, "kn", False),
            ("bias-off-by-4-bytes", 64, 64, 64, "nk", True), ("M65", 65, 64, 64, "nk", False), ("N-not-16", 64, 64, 72, "nk", False),
            ("nkt7", 65, 224, 192, "nk", False), ("nkt8", 65, 256, 192, "nk", False),
            ("tiles64", 1024, 256, 1024, "nk", False), ("tiles72", 1025, 256, 1024, "nk", False)]


def test_dispatcher_rules_hold_on_both_sides(monkeypatch):
    """functional._igemm takes the skinny kernel exactly where sp_gemm_skinny_applies holds (<= 64 rows, aligned pointers) and split-K exactly where
    tiles <= 64 and nkt >= _KSPLIT_MIN_NKT; forward and both gradients of functional.gemm inside the bar of the kernel that ran"""
    from scanpaths_amd import functional as F
    hip, L = P.abi()
    calls = []
    real_ig, real_sk = L.sp_conv_igemm, L.sp_gemm_skinny

    def spy_ig(d, *a):
        calls.append(("igemm", d._obj.ksplit))
        return real_ig(d, *a)

    def spy_sk(*a):
        calls.append(("skinny", 0))
        return real_sk(*a)
    monkeypatch.setattr(L, "sp_conv_igemm", spy_ig)
    monkeypatch.setattr(L, "sp_gemm_skinny", spy_sk)
    seen = set()
    dev = P.dev()
    for name, M, K, N, layout, bias_off in DISPATCH:
        s = P.seed_of("dispatch" + name)
        a, b = P.randn(M, K, seed=s), (P.randn(N, K, seed=s + 1) if layout == "nk" else P.randn(K, N, seed=s + 1))
        bias, gc = P.randn(N, seed=s + 2), P.randn(M, N, seed=s + 3)
        bm = b.t() if layout == "nk" else b                                                  # [K, N]
        ag, bg = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
        biasg = torch.zeros(N + 4, device=dev)[1:N + 1].copy_(bias) if bias_off else bias.to(dev)
        assert biasg.data_ptr() % 16 == (4 if bias_off else 0)
        calls.clear()
        F.reset_fusion_counts()
        out = F.gemm(ag, bg, biasg, layout, alpha=0.5)
        out.backward(gc.to(dev))
        torch.cuda.synchronize()
        # the two _igemm calls: forward (mode 0 for "nk") and data gradient (the other mode, Nout = K, Kc = N)
        expect, chains = [], []
        for (m_, n_, k_, mode, has_bias) in ((M, N, K, 0 if layout == "nk" else 1, True), (M, K, N, 1 if layout == "nk" else 0, False)):
            ldw = (K if layout == "nk" else N)
            skinny = (m_ <= 64 and not (has_bias and bias_off) and n_ % 4 == 0
                      and L.sp_gemm_skinny_applies(m_, n_, k_, k_, ldw, n_, mode) == 1)
            tiles, nkt = P.cdiv(m_, 128) * P.cdiv(n_, 128), P.cdiv(k_, 32)
            split = not skinny and tiles <= 64 and nkt >= F._KSPLIT_MIN_NKT
            ks = max(2, min(nkt // F._KSPLIT_KT, 512 // tiles)) if split else 0
            expect.append(("skinny", 0) if skinny else ("igemm", ks))
            chains.append(R.chain_skinny(n_, k_, mode) if skinny else R.chain_igemm(k_, 1, ks))
            seen.add(("skinny", skinny))
            if not skinny:
                seen.add(("split", split, "tiles<=64" if tiles <= 64 else "tiles>64", "nkt>=8" if nkt >= 8 else "nkt<8"))
        assert calls == expect, (name, calls, expect)
        assert F.FUSION_COUNTS["skinny_gemm"] == sum(e[0] == "skinny" for e in expect), (name, F.FUSION_COUNTS)
        ref, S = R.reference(a[None], bm[None], 0.5, bias)
        SUM.judge("dispatch", name + " forward", P.Guarded(1, M, N, N, fill="sentinel"), _as_guarded(out), ref, S, chains[0], _gemm_legacy(K))
        ref, S = R.reference(gc[None], bm.t()[None], 0.5)
        SUM.judge("dispatch", name + " dA", P.Guarded(1, M, K, K, fill="sentinel"), _as_guarded(ag.grad), ref, S, chains[1], _gemm_legacy(N))
        # dB = alpha dC^T A ("nk": [N, K]) or alpha A^T dC ("kn": [K, N]) on sp_conv_wgrad
        Co, Ci = (N, K) if layout == "nk" else (K, N)
        splits = R.wgrad_splits(L, F._gemm_wgrad_desc(M, Co, Ci, ldx=Ci, ldy=Co, ldo=Ci, alpha=0.5), Co, Ci)[0]
        lhs, rhs = (gc.t(), a) if layout == "nk" else (a.t(), gc)
        ref, S = R.reference(lhs[None], rhs[None], 0.5)
        SUM.judge("dispatch", name + f" dB (splits {splits})", P.Guarded(1, Co, Ci, Ci, fill="sentinel"), _as_guarded(bg.grad), ref, S,
               R.chain_wgrad(M, splits), _gemm_legacy(M))
    assert {("skinny", True), ("skinny", False)} <= seen
    assert ("split", True, "tiles<=64", "nkt>=8") in seen and ("split", False, "tiles<=64", "nkt<8") in seen and \
        ("split", False, "tiles>64", "nkt>=8") in seen, seen


def _as_guarded(t):
    """a dense result of the dispatcher in the layout SUM.judge reads: sentinel guards around the tensor's words"""
    g = torch.full((P.GUARD,), P.SENTINEL, dtype=torch.int32).view(torch.float32)
    return torch.cat([g, t.detach().cpu().reshape(-1), g])


# ====================================================================================================================
# the CHUNK comment of csrc/conv_igemm.hip: a long reduction stays within 2 x of a blocked CPU summation
# ====================================================================================================================
def _rms(x):
    return float(x.double().pow(2).mean().sqrt())


def test_long_reduction_stays_within_twice_the_cpu_fp32_error():
    """K = 18432 (the sal_conv reduction): rms error against fp64 of sp_conv_igemm (M = 128, N = 64) and of sp_conv_wgrad (18432 rows, 128 x 64) at
    most 2 x the rms error of torch's CPU fp32 matmul on the same data"""
    ig = R.IgemmProblem(R._ig("long-reduction-K18432", 128, 18432, 64, 0, alpha=1.0, bias=False))
    ref, S = ig.reference()
    flat = _run_igemm("long_reduction", ig, _gemm_legacy(18432))
    x, w = ig.X.live(ig.X.flat)[0], ig.W.live(ig.W.flat)[0]
    e_gpu, e_cpu = _rms(ig.out.live(flat)[0] - ref[0]), _rms((x @ w.t()).double() - ref[0])
    print(f"PARITY long_reduction igemm: rms err {e_gpu:.3e}, CPU fp32 matmul {e_cpu:.3e}, ratio {e_gpu / e_cpu:.2f}")
    wg = R.WgradProblem(R._wg("long-reduction-rows18432", 18432, 128, 64, alpha=1.0))
    ref, S = wg.reference()
    flat = _run_wgrad("long_reduction", wg, _gemm_legacy(18432))
    x, dy = wg.X.live(wg.X.flat)[0], wg.dY.live(wg.dY.flat)[0]
    w_gpu, w_cpu = _rms(wg.out.live(flat)[0] - ref[0]), _rms((dy.t() @ x).double() - ref[0])
    print(f"PARITY long_reduction wgrad: rms err {w_gpu:.3e}, CPU fp32 matmul {w_cpu:.3e}, ratio {w_gpu / w_cpu:.2f}")
    assert e_gpu <= 2.0 * e_cpu, (e_gpu, e_cpu)
    assert w_gpu <= 2.0 * w_cpu, (w_gpu, w_cpu)
