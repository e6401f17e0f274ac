"""Decoder, loss and optimizer kernels (csrc/decoder.hip, csrc/loss_opt.hip, the rowsum pair of csrc/bn_pool.hip) at the shapes their one
friendly op-level case never reaches: every HIP op -- through scanpaths_amd.functional or the ctypes ABI -- against a plain torch fp64 CPU
restatement of the same lines of the reference, forward and every input gradient.

Bars: ordinary-magnitude cases use the bar tests/test_ops_gpu.py already holds the op to, with the same metric (parity.close: max error over
max(1, max |ref|)).  Stress cases (scores / logits spanning tens of units, where expf's error grows with its argument) use the rule of
tests/test_salmaps_gpu.py: bar = max(existing bar, 10 x max|ref32 - ref64|), ref32 = the SAME restatement in fp32 on the CPU -- both sides
of that difference come from the reference, never from the kernel; the factor 10 is the margin for another summation order.
Wherever a ReLU sits between an input and a gradient, the fp64 side asserts |pre| >= 1e-4 max|pre| for EVERY pre-activation (no
exclusions), so a flipped mask cannot be explained away.  Every test prints its worst err / bar (profiles/decoder_ops_parity.md)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from parity import Worst, dev as _dev, rand as _rand, stress_bar

pytestmark = pytest.mark.gpu

HC = 64


def _leaf(t, dtype):
    """a fresh leaf of the reference side (t.to(float32) alone would alias the fp32 input and mark IT as requiring grad)"""
    return t.detach().clone().to(dtype).requires_grad_(True)


def _away(x, lo):
    """the same signs, magnitudes moved away from zero by lo"""
    return torch.where(x >= 0, x + lo, x - lo)


def _margin(pre, what):
    """no pre-activation of a ReLU within 1e-4 of the largest one of zero: a mask flip in fp32 is then a defect, not rounding"""
    pre = pre.detach().double()
    lo, hi = pre.abs().min().item(), pre.abs().max().item()
    assert lo >= 1e-4 * hi, f"{what}: min |pre| {lo:.3e} < 1e-4 x max |pre| {hi:.3e}: pick another seed"


# ====================================================================================================================
# attention over a memory list
# ====================================================================================================================
def _att_ref(Lst, u, gm, dtype):
    """spatial / semantic attention of AiR/models/baseline_attention.py:67-88, 99-123 on the memory list: scores <L[t, r], u>, softmax over the
    list, weighted sum of the entries"""
    Lr, ur = _leaf(Lst, dtype), _leaf(u, dtype)
    sc = (Lr * ur).sum(-1)
    mem = (Lr * sc.softmax(0).unsqueeze(-1)).sum(0)
    mem.backward(gm.to(dtype))
    return mem.detach(), Lr.grad, ur.grad


def _att_hip(Lst, u, gm):
    from scanpaths_amd import functional as F
    dev = _dev()
    Lg, ug = Lst.to(dev).requires_grad_(True), u.to(dev).requires_grad_(True)
    mem = F.list_attention(Lg, ug)
    mem.backward(gm.to(dev))
    return mem.detach(), Lg.grad, ug.grad


ATT_CASES = [(1, 1, 1), (1, 3, 256), (4, 2, 255), (8, 1, 257), (16, 4, 2560), (39, 2, 64), (40, 3, 513)]


@pytest.mark.parametrize("T,R,D", ATT_CASES)
def test_list_attention_at_edge_shapes(T, R, D):
    """listatt_fwd/bwd_kernel (baseline_attention.py:67-88, 99-123): T = 1, T a multiple of 4 (four entries per reduction round), T = MAXT
    and MAXT - 1, D below / at / around one 256-thread pass.  T = 1: the softmax is exactly 1, so mem is L[0], dL is dmem and du is 0, bit
    for bit.  Two calls give identical bits."""
    w = Worst(f"list_attention T={T} R={R} D={D}")
    Lst, u, gm = _rand(T, R, D, seed=11), _rand(D, seed=12, scale=1.5 / math.sqrt(D)), _rand(R, D, seed=13)
    memr, dLr, dur = _att_ref(Lst, u, gm, torch.float64)
    mem, dL, du = _att_hip(Lst, u, gm)
    w.close(mem, memr, 3e-6, "mem")
    w.close(dL, dLr, 1e-5, "dL")
    w.close(du, dur, 1e-5, "du")
    mem2, dL2, du2 = _att_hip(Lst, u, gm)
    assert torch.equal(mem2, mem) and torch.equal(dL2, dL) and torch.equal(du2, du)
    if T == 1:
        assert torch.equal(mem.cpu(), Lst[0]) and torch.equal(dL.cpu()[0], gm)
        assert float(du.abs().max()) == 0.0
    w.report()


@pytest.mark.parametrize("kind", ["scores_span_60", "identical_entries"])
def test_list_attention_stress(kind):
    """one dominant score (the scores of row 0 span about +-60: the softmax saturates, exp of the others underflows towards 0) and T
    identical entries (all weights 1/T, the score gradient a difference of equal numbers).  Bars by the ref32 rule."""
    T, R, D = 8, 3, 513
    w = Worst(f"list_attention {kind}")
    Lst, u, gm = _rand(T, R, D, seed=21), _rand(D, seed=22, scale=1.5 / math.sqrt(D)), _rand(R, D, seed=23)
    if kind == "scores_span_60":
        sc = (Lst.double() * u.double()).sum(-1)[:, 0]
        u = (u.double() * (60.0 / sc.abs().max())).float()
        sc = (Lst.double() * u.double()).sum(-1)[:, 0]
        assert 59.0 <= sc.abs().max().item() <= 61.0 and sc.max().item() - sc.min().item() > 60.0
    else:
        Lst = Lst[:1].expand(T, R, D).contiguous()
    r64, r32 = _att_ref(Lst, u, gm, torch.float64), _att_ref(Lst, u, gm, torch.float32)
    got = _att_hip(Lst, u, gm)
    for g, a, b, base, what in zip(got, r32, r64, (3e-6, 1e-5, 1e-5), ("mem", "dL", "du")):
        w.close(g, b, stress_bar(base, a, b), what)
    w.report()


# ====================================================================================================================
# semantic pooling
# ====================================================================================================================
# seeds for which every pre-activation keeps the 1e-4 margin (checked on the fp64 side by _margin below, on every run)
POOL_CASES = [(1, 1, 1, 4, 0), (2, 1, 159, 8, 0), (2, 2, 160, 512, 1), (1, 3, 161, 260, 0), (2, 2, 321, 128, 2)]


def _pool_inputs(S, B, P, C, seed):
    return _rand(S, B, P, seed=100 + seed).abs(), _rand(B, P, C, seed=200 + seed), _rand(B, S, C, seed=300 + seed)


def _pool_ref(a, vf, g):
    """get_channel_semantic + ReLU, baseline_attention.py:246-250, 284, 324: relu(mean_p(a[s, b, p] vf[b, p, :]))"""
    P = a.shape[-1]
    ar, vr = a.double().requires_grad_(True), vf.double().requires_grad_(True)
    pre = torch.einsum("sbp,bpc->bsc", ar, vr) / P
    ref = torch.relu(pre)
    (ref * g.double()).sum().backward()
    return ref.detach(), ar.grad, vr.grad, pre.detach()


@pytest.mark.parametrize("sbc", [False, True])
@pytest.mark.parametrize("S,B,P,C,seed", POOL_CASES)
def test_semantic_pool_at_edge_shapes(S, B, P, C, seed, sbc):
    """sempool_fwd / finish / bwd kernels (baseline_attention.py:246-250, 284, 324): one pixel, one chunk of SP_PCH = 160 pixels less one /
    exactly / plus one, three chunks, C = 4 (one channel quad), C = 260 (a second quad round of the backward wave; not a multiple of 256),
    C = 512 (every thread of the forward block).  The [S,B,C] form is bit-equal to the [B,S,C] one."""
    from scanpaths_amd import functional as F
    w = Worst(f"semantic_pool S={S} B={B} P={P} C={C} sbc={sbc}")
    a, vf, g = _pool_inputs(S, B, P, C, seed)
    ref, dar, dvr, pre = _pool_ref(a, vf, g)
    _margin(pre, "pooled")
    dev = _dev()
    ad, vd = a.to(dev).requires_grad_(True), vf.to(dev).requires_grad_(True)
    out = F.semantic_pool(ad, vd)
    (out * g.to(dev)).sum().backward()
    a2, v2 = a.to(dev).requires_grad_(True), vf.to(dev).requires_grad_(True)
    out2 = F.semantic_pool(a2, v2, sbc=True)
    (out2 * g.to(dev).transpose(0, 1)).sum().backward()
    assert out2.shape == (S, B, C) and torch.equal(out2.transpose(0, 1), out)
    assert torch.equal(a2.grad, ad.grad) and torch.equal(v2.grad, vd.grad)
    o, da, dv = (out2.transpose(0, 1), a2.grad, v2.grad) if sbc else (out, ad.grad, vd.grad)
    w.close(o, ref, 3e-6, "pooled")
    w.close(da, dar, 3e-6, "d amaps")
    w.close(dv, dvr, 3e-6, "d vf")
    w.report()


@pytest.mark.parametrize("sbc", [0, 1])
def test_semantic_pool_backward_writes_exact_zeros_for_dead_samples(sbc):
    """sempool_bwd_kernel's row_last branch through the ABI: a sample whose last loss step lies before this memory update receives exact
    zeros and none of its inputs is read (its vf and dz rows are NaN here); the live samples are bit-equal to the dense call."""
    from scanpaths_amd import hip
    from scanpaths_amd.functional import check
    S, B, P, C, step = 2, 3, 161, 260, 4
    dev, L = _dev(), hip.lib()
    a, vf, g = (t.to(dev) for t in _pool_inputs(S, B, P, C, 1))
    dz = (g if not sbc else g.transpose(0, 1)).contiguous()
    out = torch.empty_like(dz)
    ws = torch.empty(L.sp_sempool_workspace(S, B, P, C), dtype=torch.uint8, device=dev)
    check(L.sp_sempool_fwd(hip.ptr(a), hip.ptr(vf), S, B, P, C, 1.0 / P, hip.ptr(ws), hip.ptr(out), sbc, hip.stream()), "sp_sempool_fwd")

    def run(vf_, dz_, last):
        da, dvf = torch.full_like(a, float("nan")), torch.full_like(vf, float("nan"))
        check(L.sp_sempool_bwd(hip.ptr(dz_), hip.ptr(out), hip.ptr(a), hip.ptr(vf_), S, B, P, C, 1.0 / P, hip.ptr(da), hip.ptr(dvf),
                               hip.ptr(last) if last is not None else None, step, sbc, hip.stream()), "sp_sempool_bwd")
        torch.cuda.synchronize()
        return da, dvf
    da, dvf = run(vf, dz, None)
    assert bool(torch.isfinite(da).all()) and bool(torch.isfinite(dvf).all())
    last = torch.tensor([step - 1, step, step + 3], dtype=torch.int32, device=dev)
    vfn, dzn = vf.clone(), dz.clone()
    vfn[0] = float("nan")
    if sbc:
        dzn[:, 0] = float("nan")
    else:
        dzn[0] = float("nan")
    da2, dvf2 = run(vfn, dzn, last)
    assert float(da2[:, 0].abs().max()) == 0.0 and float(dvf2[0].abs().max()) == 0.0
    assert torch.equal(da2[:, 1:], da[:, 1:]) and torch.equal(dvf2[1:], dvf[1:])
    # and against fp64 (the dense call)
    _, dar, dvr, pre = _pool_ref(a.cpu(), vf.cpu(), g.cpu())
    _margin(pre, "pooled")
    w = Worst(f"semantic_pool row_last sbc={sbc}")
    w.close(da, dar, 3e-6, "d amaps")
    w.close(dvf, dvr, 3e-6, "d vf")
    w.report()


# ====================================================================================================================
# im2col of the 1-channel maps and its adjoint
# ====================================================================================================================
def _im2col_ref(maps, KP):
    """the 3x3 pad-1 window of every stream's map (the operand of the rank-1 gate term, baseline_attention.py:40-50), stream s in columns
    [9 s, 9 s + 9), zero columns behind"""
    S, R, H, W_ = maps.shape
    cols = [TF.unfold(maps[s][:, None], 3, padding=1).transpose(1, 2) for s in range(S)]          # [R, H*W, 9] each
    pad = maps.new_zeros(R, H * W_, KP - 9 * S)
    return torch.cat(cols + [pad], -1)


@pytest.mark.parametrize("S,R,H,W_,KP", [(1, 1, 1, 1, 9), (1, 2, 1, 7, 12), (2, 3, 5, 1, 20), (2, 2, 6, 8, 20), (3, 1, 4, 5, 32)])
def test_im2col3x3_and_its_adjoint(S, R, H, W_, KP):
    """im2col1_multi_kernel / col2im1_multi_kernel: one to three streams, no padding columns (KP = 9) and some, 1 x 1 / 1 x N / N x 1 maps
    (every tap but the centre column / row falls into the zero padding).  Forward is a gather: equal bits; the adjoint sums <= 9 values."""
    from scanpaths_amd import functional as F
    w = Worst(f"im2col3x3 S={S} R={R} {H}x{W_} KP={KP}")
    maps, g = _rand(S, R, H, W_, seed=31), _rand(R, H * W_, KP, seed=32)
    ref = _im2col_ref(maps, KP)
    mr = maps.double().requires_grad_(True)
    (_im2col_ref(mr, KP) * g.double()).sum().backward()
    dev = _dev()
    md = maps.to(dev).requires_grad_(True)
    col = F.im2col3x3(md, KP)
    (col * g.to(dev)).sum().backward()
    assert col.shape == (R, H * W_, KP) and torch.equal(col.cpu(), ref)
    if KP > 9 * S:
        assert float(col.detach()[..., 9 * S:].abs().max()) == 0.0
    w.close(md.grad, mr.grad, 1e-6, "d maps")
    w.report()


# ====================================================================================================================
# head epilogue
# ====================================================================================================================
def _sites(n):
    return (n + 4 - 7) // 5 + 1


def _head_inputs(Hm, Wm, nh, per_sample, zc, extra=0, seed=0, B=2):
    """Z [B, Hm, Wm, nh * zc + extra], composed biases, drt_layer_2, duration-site window sums (zc = 2) -- the action-map column and the
    window sums are moved away from zero (they feed ReLUs)"""
    S = _sites(Hm) * _sites(Wm)
    Z = _rand(B, Hm, Wm, nh * zc + extra, seed=seed + 1)
    for hd in range(nh):
        Z[..., hd * zc + 1] = _away(Z[..., hd * zc + 1], 1.0)
    cb = _rand(*((B, nh, HC) if per_sample else (nh, HC)), seed=seed + 2, scale=0.1)
    w2, b2 = _rand(2, S, seed=seed + 3, scale=0.5 / math.sqrt(S)), _rand(2, seed=seed + 4, scale=0.1)
    dpre = _away(_rand(nh, B, S, seed=seed + 5), 1.0) if zc == 2 else None
    return Z, cb, w2, b2, dpre


def _head_ref(Z, cb, w2, b2, dpre, nh, zc, softmax, per_sample, cots, dtype):
    """predict_head behind its 5x5 conv, restated from Z (baseline_attention.py:149-158 with the heads composed, scanpath_model._compose_heads):
    term = mean(z0) + c0, amap = relu(z1 + c1), drt = relu(dpre + c51) with dpre either given or the 7x7 stride-5 pad-2 conv of the
    intermediate map (tap k reads column 2 + k: a one-hot depth filter; padding taps carry neither value nor bias), mu = <w2[0], drt> + b2[0],
    sigma2 = exp(<w2[1], drt> + b2[1]), logits = [term, amap] (softmax over the 1 + P actions when asked)."""
    B, Hm, Wm, _ = Z.shape
    P, S = Hm * Wm, _sites(Hm) * _sites(Wm)
    leaves = [_leaf(t, dtype) if t is not None else None for t in (Z, cb, w2, b2, dpre)]
    Zr, cbr, w2r, b2r, dr = leaves
    lg, am, mu, s2, pres = [], [], [], [], []
    for hd in range(nh):
        z = Zr[..., hd * zc:(hd + 1) * zc].reshape(B, P, zc)
        c = cbr[:, hd] if per_sample else cbr[hd].expand(B, HC)
        term = z[:, :, 0].mean(1) + c[:, 0]
        pa = z[:, :, 1] + c[:, 1:2]
        a = torch.relu(pa)
        pres.append(pa)
        l = torch.cat([term[:, None], a], 1)
        lg.append(l.softmax(1) if softmax else l)
        am.append(a)
        if dr is not None:
            pd = dr[hd] + c[:, 51:52]
        else:
            inter = (z[:, :, 2:51] + c[:, None, 2:51]).reshape(B, Hm, Wm, 49).permute(0, 3, 1, 2)
            eye = torch.eye(49, dtype=dtype).view(1, 49, 7, 7)
            pd = TF.conv2d(inter, eye, None, stride=5, padding=2).reshape(B, S) + c[:, 51:52]
        d = torch.relu(pd)
        pres.append(pd)
        mu.append(d @ w2r[0] + b2r[0])
        s2.append(torch.exp(d @ w2r[1] + b2r[1]))
    outs = [torch.stack(lg), torch.stack(am), torch.stack(mu), torch.stack(s2)]
    sum((o * g.to(dtype)).sum() for o, g in zip(outs, cots)).backward()
    grads = [t.grad if t is not None else None for t in leaves]
    return [o.detach() for o in outs], grads, pres


def _head_cots(B, P, nh, seed):
    return [_rand(nh, B, P + 1, seed=seed + 6), _rand(nh, B, P, seed=seed + 7), _rand(nh, B, seed=seed + 8), _rand(nh, B, seed=seed + 9)]


def _head_hip(Z, cb, w2, b2, dpre, nh, softmax, per_sample, cots):
    from scanpaths_amd import functional as F
    dev = _dev()
    leaves = [t.to(dev).requires_grad_(True) if t is not None else None for t in (Z, cb, w2, b2, dpre)]
    outs = F.head_finish(leaves[0], leaves[1], leaves[2], leaves[3], nh, HC, softmax, per_sample=per_sample, dpre=leaves[4])
    sum((o * g.to(dev)).sum() for o, g in zip(outs, cots)).backward()
    return [o.detach() for o in outs], [t.grad if t is not None else None for t in leaves]


_OUT_NAMES, _OUT_BARS = ("logits", "amap", "mu", "sigma2"), (2e-5, 2e-5, 2e-5, 5e-5)
_GRAD_NAMES = ("dZ", "dcb", "dw2", "db2", "ddpre")


def _head_compare(w, got, ref, r32=None):
    (o, g), (o64, g64, _) = got, ref
    for k, name in enumerate(_OUT_NAMES[:len(o64)]):
        w.close(o[k], o64[k], _OUT_BARS[k] if r32 is None else stress_bar(_OUT_BARS[k], r32[0][k], o64[k]), name)
    for k, name in enumerate(_GRAD_NAMES):
        if g64[k] is not None:
            w.close(g[k], g64[k], 3e-5 if r32 is None else stress_bar(3e-5, r32[1][k], g64[k]), name)


_ALL = [(1, False, False), (2, True, True), (2, False, True), (1, True, False)]        # (nheads, per_sample, softmax): every value of every axis
_TWO = [(2, False, True), (1, True, False)]
HEAD_SIZES = [((3, 3), _ALL), ((7, 8), _TWO), ((12, 13), _TWO), ((16, 15), _ALL), ((15, 17), _ALL), ((16, 16), _ALL), ((78, 78), _TWO)]
HEAD_CASES = [(hw, nh, ps, sm) for hw, combos in HEAD_SIZES for nh, ps, sm in combos]


@pytest.mark.parametrize("hw,nh,per_sample,softmax", HEAD_CASES)
def test_head_finish_at_edge_shapes(hw, nh, per_sample, softmax):
    """head_fwd/bwd_kernel with the duration-site sums given (dpre, zc = 2), the form the model runs: 1 + P = 10, 57, 157, then 241 / 256 / 257
    around one 256-thread pass of the softmax loops, and 78 x 78 with S = MAXS = 256 duration sites; S = 1 at 3 x 3.  softmax = True forward AND
    backward (the RL phase differentiates it), one and two heads, shared and per-sample composed biases; cotangents on all four outputs."""
    Hm, Wm = hw
    w = Worst(f"head_finish {Hm}x{Wm} nh={nh} per_sample={per_sample} softmax={softmax}")
    ins = _head_inputs(Hm, Wm, nh, per_sample, 2, seed=40)
    cots = _head_cots(2, Hm * Wm, nh, 40)
    ref = _head_ref(*ins, nh, 2, softmax, per_sample, cots, torch.float64)
    for k, pre in enumerate(ref[2]):
        _margin(pre, f"pre-activation {k}")
    _head_compare(w, _head_hip(*ins, nh, softmax, per_sample, cots), ref)
    w.report()


def test_head_finish_with_wider_rows_leaves_the_unused_columns_zero():
    """ldz = used columns + 6: the kernel addresses rows by ldz and dZ's columns behind the heads' are exact zeros"""
    Hm, Wm, nh = 7, 8, 2
    w = Worst("head_finish ldz = used + 6")
    ins = _head_inputs(Hm, Wm, nh, False, 2, extra=6, seed=50)
    cots = _head_cots(2, Hm * Wm, nh, 50)
    ref = _head_ref(*ins, nh, 2, True, False, cots, torch.float64)
    for k, pre in enumerate(ref[2]):
        _margin(pre, f"pre-activation {k}")
    got = _head_hip(*ins, nh, True, False, cots)
    assert got[1][0].shape[-1] == nh * 2 + 6 and float(got[1][0][..., nh * 2:].abs().max()) == 0.0
    assert float(ref[1][0][..., nh * 2:].abs().max()) == 0.0
    _head_compare(w, got, ref)
    w.report()


# seeds for which the S duration-site sums keep the 1e-4 margin (asserted on every run)
@pytest.mark.parametrize("hw,nh,per_sample,softmax,seed", [((7, 8), 1, False, False, 60), ((7, 8), 2, True, True, 60), ((12, 13), 2, False, True, 60),
                                                           ((12, 13), 1, True, False, 60), ((16, 16), 2, True, False, 60),
                                                           ((16, 16), 1, False, True, 60)])
def test_head_finish_without_dpre_sums_the_49_taps_itself(hw, nh, per_sample, softmax, seed):
    """head_finish(dpre=None): an exported ABI path no model code calls (zc = HC = 64, Z carries the 49 tap columns of the composed 7x7
    stride-5 pad-2 duration conv).  Duration sites by the one-hot conv test_direct_head_matches_two_conv_formulation uses, so the padding
    semantics (a tap outside the intermediate map carries neither value nor composed bias) are the reference's; the gradients include
    dcb[2:51] (a sum over the sites at which the tap is inside) and dZ[..., 2:51] (the scatter of the site gradients)."""
    Hm, Wm = hw
    w = Worst(f"head_finish dpre=None {Hm}x{Wm} nh={nh} per_sample={per_sample} softmax={softmax}")
    ins = _head_inputs(Hm, Wm, nh, per_sample, HC, seed=seed)
    assert ins[4] is None and ins[0].shape[-1] == nh * HC
    cots = _head_cots(2, Hm * Wm, nh, seed)
    ref = _head_ref(*ins, nh, HC, softmax, per_sample, cots, torch.float64)
    for k, pre in enumerate(ref[2]):
        _margin(pre, f"pre-activation {k}")
    dcb = ref[1][1].reshape(-1, nh, HC)
    assert float(dcb[..., 2:51].abs().max()) > 0.0 and float(ref[1][0].reshape(2, -1, nh, HC)[..., 2:51].abs().max()) > 0.0
    assert float(dcb[..., 52:].abs().max()) == 0.0
    _head_compare(w, _head_hip(*ins, nh, softmax, per_sample, cots), ref)
    w.report()


def test_head_finish_softmax_stress():
    """logits spanning about +-40 (terminate logit near -40, action map up to +40): the softmax saturates on a few pixels; bars by the ref32
    rule"""
    Hm, Wm, nh = 15, 17, 2
    w = Worst("head_finish softmax logits span 80")
    Z, cb, w2, b2, dpre = _head_inputs(Hm, Wm, nh, False, 2, seed=70)
    for hd in range(nh):
        Z[..., hd * 2 + 1] *= 40.0 / Z[..., hd * 2 + 1].abs().max()
        Z[..., hd * 2] -= 40.0
    ins = (Z, cb, w2, b2, dpre)
    cots = _head_cots(2, Hm * Wm, nh, 70)
    ref = _head_ref(*ins, nh, 2, True, False, cots, torch.float64)
    r32 = _head_ref(*ins, nh, 2, True, False, cots, torch.float32)
    for k, pre in enumerate(ref[2]):
        _margin(pre, f"pre-activation {k}")
    pre_sm = torch.cat([Z[..., 0].reshape(2, -1).double().mean(1, keepdim=True) + cb[0, 0].double(), ref[0][1][0]], 1)
    assert pre_sm.min().item() < -39.0 and pre_sm.max().item() > 39.0
    _head_compare(w, _head_hip(*ins, nh, True, False, cots), ref, r32)
    w.report()


@pytest.mark.parametrize("hw,nh,per_sample,softmax", HEAD_CASES)
def test_head_sal_reads_its_logit_gradient_in_place(hw, nh, per_sample, softmax):
    """the saliency part alone (parts = 1), as the decode loop runs it per step: the logits of T = 2 steps are stacked to [nh, B, T, 1 + P] and
    the gradient of each step's logits is a strided slice of the stacked gradient, read in place (dl_ld).  Same sizes and axes as
    test_head_finish_at_edge_shapes."""
    from scanpaths_amd import functional as F
    Hm, Wm = hw
    B, P, T = 2, Hm * Wm, 2
    w = Worst(f"head_sal {Hm}x{Wm} nh={nh} per_sample={per_sample} softmax={softmax}")
    dev = _dev()
    G, GA = _rand(nh, B, T, P + 1, seed=86), _rand(T, nh, B, P, seed=87)
    Zs = [_head_inputs(Hm, Wm, nh, per_sample, 2, seed=80 + 3 * t)[0] for t in range(T)]
    cb = _head_inputs(Hm, Wm, nh, per_sample, 2, seed=80)[1]
    # fp64
    cbr = cb.double().requires_grad_(True)
    Zr = [z.double().requires_grad_(True) for z in Zs]
    lgs, ams = [], []
    for t in range(T):
        z = Zr[t].reshape(B, P, nh, 2)
        c = cbr.transpose(0, 1) if per_sample else cbr[:, None].expand(nh, B, HC)          # [nh, B, HC]
        term = z[..., 0].mean(1).transpose(0, 1) + c[..., 0]                                 # [nh, B]
        pa = z[..., 1].permute(2, 0, 1) + c[..., 1:2]                                        # [nh, B, P]
        _margin(pa, "action map")
        a = torch.relu(pa)
        l = torch.cat([term[..., None], a], -1)
        lgs.append(l.softmax(-1) if softmax else l)
        ams.append(a)
    ((torch.stack(lgs, 2) * G.double()).sum() + (torch.stack(ams) * GA.double()).sum()).backward()
    # HIP
    cbd = cb.to(dev).requires_grad_(True)
    Zd = [z.to(dev).requires_grad_(True) for z in Zs]
    outs = [F.head_sal(Zd[t], cbd, nh, HC, softmax, per_sample=per_sample) for t in range(T)]
    seen = []
    outs[0][0].register_hook(lambda g: seen.append((g.stride(), g.is_contiguous())))
    stacked = torch.stack([o[0] for o in outs], 2)
    ((stacked * G.to(dev)).sum() + (torch.stack([o[1] for o in outs]) * GA.to(dev)).sum()).backward()
    assert seen and seen[0][0][2] == 1 and seen[0][0][1] == T * (P + 1) and not seen[0][1], seen      # a slice of the stacked gradient
    for t in range(T):
        w.close(outs[t][0], lgs[t], 2e-5, f"logits[{t}]")
        w.close(outs[t][1], ams[t], 2e-5, f"amap[{t}]")
        w.close(Zd[t].grad, Zr[t].grad, 3e-5, f"dZ[{t}]")
    w.close(cbd.grad, cbr.grad, 3e-5, "dcb")
    w.report()


# ====================================================================================================================
# elementwise
# ====================================================================================================================
def test_mul_relu_beyond_the_block_cap():
    """mulrelu_fwd/bwd_kernel (get_spatial_semantic, baseline_attention.py:252-256): n = 2 x (2048 x 256 + 3) elements, more than the 2048 blocks
    of 256 threads cover in one pass (grid-stride loop), the broadcast b[i % nb] crossing the wrap"""
    from scanpaths_amd import functional as F
    n = 2048 * 256 + 3
    w = Worst(f"mul_relu a=(2, {n})")
    a, b, go = _away(_rand(2, n, seed=91), 0.5), _away(_rand(n, seed=92), 0.5), _rand(2, n, seed=93)
    ar, br = a.double().requires_grad_(True), b.double().requires_grad_(True)
    pre = ar * br
    _margin(pre, "a * b")
    outr = torch.relu(pre)
    outr.backward(go.double())
    dev = _dev()
    ag, bg = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    out = F.mul_relu(ag, bg)
    out.backward(go.to(dev))
    w.close(out, outr, 1e-6, "out")
    w.close(ag.grad, ar.grad, 1e-6, "da")
    w.close(bg.grad, br.grad, 1e-6, "db")
    w.report()


@pytest.mark.parametrize("ln", [1, 33])
def test_select_rows_beyond_the_block_cap(ln):
    """select_rows_kernel and its adjoint with rows x len just above 2048 x 256 (grid-stride loop): a copy, so equal bits"""
    from scanpaths_amd import functional as F
    rows = (2048 * 256) // ln + 1
    assert 2048 * 256 < rows * ln <= 2048 * 256 + ln
    a, b, g = _rand(rows, ln, seed=94), _rand(rows, ln, seed=95), _rand(rows, ln, seed=96)
    sel = torch.from_numpy(np.random.Generator(np.random.PCG64(97)).integers(0, 2, rows).astype(bool))
    dev = _dev()
    ag, bg = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    o = F.select_rows(ag, bg, sel.to(dev))
    o.backward(g.to(dev))
    zero = torch.zeros_like(g)
    assert torch.equal(o.cpu(), torch.where(sel[:, None], a, b))
    assert torch.equal(ag.grad.cpu(), torch.where(sel[:, None], g, zero))
    assert torch.equal(bg.grad.cpu(), torch.where(sel[:, None], zero, g))
    print(f"PARITY select_rows rows={rows} len={ln}: worst err/bar 0.000 (bit-equal)")


@pytest.mark.parametrize("C,M", [(4, 1), (4, 5), (4, 16385), (252, 1), (252, 5), (256, 1), (256, 5), (260, 1), (260, 5), (2048, 1), (2048, 5)])
def test_channel_mean_at_edge_shapes(C, M):
    """rowsum_kernel / rowsum_bwd_kernel (mean over channels of the visual feature, baseline_attention.py:252-256): one float4 per row (C = 4),
    one 256-wide wave pass less / exactly / plus a quad, eight passes; M = 16385 rows = one more than the 4096 blocks x 4 waves of the capped
    grid take in one round"""
    from scanpaths_amd import functional as F
    w = Worst(f"channel_mean C={C} M={M}")
    x, g = _rand(M, C, seed=98), _rand(M, seed=99)
    xr = x.double().requires_grad_(True)
    mr = xr.mean(-1)
    mr.backward(g.double())
    dev = _dev()
    xg = x.to(dev).requires_grad_(True)
    m = F.channel_mean(xg)
    m.backward(g.to(dev))
    w.close(m, mr, 1e-6, "mean")
    w.close(xg.grad, xr.grad, 1e-6, "dx")
    w.report()


# ====================================================================================================================
# supervised loss
# ====================================================================================================================
def _loss_inputs(B, T, A, stress=False):
    """hand-built rows: a two-entry soft target, a target on class 0 (terminate), a row with action mask 0, a row with duration mask 0,
    a duration of exactly 0, sigma2 in {1e-3, 10}"""
    R = B * T
    z = _rand(R, A, seed=110) * 2
    mu, s2 = _rand(R, seed=111), torch.full((R,), 10.0)
    s2[::2] = 1e-3
    dur = _rand(R, seed=112).abs() * 0.3 + 0.05
    gt = torch.zeros(R, A)
    am, dm = torch.ones(R), torch.ones(R)
    tgt = [(3 * r + 1) % A for r in range(R)]
    for r in range(R):
        gt[r, tgt[r]] = 1.0
    gt[0] = 0.0
    gt[0, 0], gt[0, A - 1] = 0.3, 0.7                    # two-entry soft target (one entry on the terminate class, one on the last class)
    dur[0] = 0.0                                          # duration exactly 0 (with sigma2 = 1e-3)
    if R > 1:
        gt[1] = 0.0
        gt[1, 0] = 1.0                                    # target on class 0
        dm[1] = 0.0                                       # ... whose duration is masked (the scanpath ended)
        am[2], dm[2] = 0.0, 0.0                           # a fully masked row
        dur[3] = 0.0                                      # duration exactly 0 with sigma2 = 10
        dm[5] = 0.0                                       # duration mask 0 under an action mask 1 (row 4: sigma2 = 1e-3, duration > 0)
    if stress:
        r = R - 1
        z[r] -= z[r].max()
        z[r, tgt[r]] = -100.0                             # the target's probability underflows in fp32
    shape = lambda t: t.view(B, T, *t.shape[1:]).contiguous()
    return tuple(shape(t) for t in (z, mu, s2, gt, am, dur, dm))


def _loss_ref(z, mu, s2, gt, am, dur, dm, lam, dtype):
    """CrossEntropyLoss AiR/models/loss.py:10-14, MLPLogNormalDistribution loss.py:27-32, loss = L_a + lambda_1 L_d AiR/train.py:192-197"""
    from oracle import scanpath_oracle as O
    zr, mur, s2r = (_leaf(t, dtype) for t in (z, mu, s2))
    batch = {"scanpaths": gt.to(dtype), "action_masks": am.to(dtype), "durations": dur.to(dtype), "duration_masks": dm.to(dtype)}
    loss, la, ld = O.supervised_loss({"all_actions_prob": zr, "log_normal_mu": mur, "log_normal_sigma2": s2r}, batch, lambda_1=lam)
    (loss * 1.7).backward()
    return [loss.detach(), la.detach(), ld.detach(), zr.grad, mur.grad, s2r.grad]


def _loss_hip(z, mu, s2, gt, am, dur, dm, lam):
    from scanpaths_amd import functional as F
    dev = _dev()
    zg, mug, s2g = (t.to(dev).requires_grad_(True) for t in (z, mu, s2))
    sums = torch.stack([am.sum(), dm.sum()]).to(dev)                      # explicit mask sums (what a data-parallel caller passes)
    loss, la, ld = F.scanpath_loss(zg, mug, s2g, gt.to(dev), am.to(dev), dur.to(dev), dm.to(dev), lam, mask_sums=sums)
    (loss * 1.7).backward()
    return [loss.detach(), la.detach(), ld.detach(), zg.grad, mug.grad, s2g.grad]


_LOSS_NAMES = ("loss", "loss_actions", "loss_duration", "dz", "dmu", "dsigma2")


@pytest.mark.parametrize("B,T,A", [(1, 1, 2), (2, 3, 255), (2, 3, 256), (2, 3, 257)])
def test_scanpath_loss_on_hand_built_rows(B, T, A):
    """loss_rows_kernel / loss_final_kernel (loss.py:10-14, 27-32; train.py:192-197) against oracle.supervised_loss in fp64: A = 2 and one
    256-thread pass less / exactly / plus one class; soft and terminate targets, masked rows, duration 0, sigma2 1e-3 and 10, lambda_1 =
    0.37, explicit mask sums.  Masked rows receive exact zeros."""
    w = Worst(f"scanpath_loss B={B} T={T} A={A}")
    ins = _loss_inputs(B, T, A)
    ref, got = _loss_ref(*ins, 0.37, torch.float64), _loss_hip(*ins, 0.37)
    for g, r, name in zip(got, ref, _LOSS_NAMES):
        w.close(g, r, 2e-6, name)
    if B * T > 1:
        dz, dmu, ds2 = (t.reshape(B * T, -1) for t in got[3:])
        assert float(dz[2].abs().max()) == 0.0 and float(dmu[[1, 2, 5]].abs().max()) == 0.0 and float(ds2[[1, 2, 5]].abs().max()) == 0.0
    w.report()


def test_scanpath_loss_with_an_underflowing_target_probability():
    """one row whose target logit lies 100 below the row maximum: p underflows in fp32, log(p + eps) is log(eps); bars by the ref32 rule"""
    w = Worst("scanpath_loss target logit 100 below the maximum")
    ins = _loss_inputs(2, 3, 257, stress=True)
    ref, r32, got = _loss_ref(*ins, 0.37, torch.float64), _loss_ref(*ins, 0.37, torch.float32), _loss_hip(*ins, 0.37)
    for g, a, r, name in zip(got, r32, ref, _LOSS_NAMES):
        w.close(g, r, stress_bar(2e-6, a, r), name)
    w.report()


# ====================================================================================================================
# reductions and Adam through the ABI
# ====================================================================================================================
def _cancelling(n, seed):
    """pairs +-1e4 (1 + u) in a seeded order plus a small remainder: the sum is ~1e-8 of sum |x|"""
    g = np.random.Generator(np.random.PCG64(seed + n))
    m = (n - 1) // 2
    big = (1e4 * (1.0 + g.random(m))).astype(np.float32)
    x = np.concatenate([big, -big, np.array([0.37, -0.11], np.float32)[:n - 2 * m]])
    return torch.from_numpy(x[g.permutation(n)])


@pytest.mark.parametrize("n", [1, 255, 1025, 1024 * 1024 + 5])
def test_sum_and_sumsq_of_cancelling_data(n):
    """reduce_partial<., .> + reduce_final_*: one element, less than a block, one more than a block's 1024-element share, beyond the cap of
    1024 blocks (grid-stride loop).  The kernels accumulate in double: sumsq (a double) within 1e-12 relative of the exact sum; sum (a
    float) within 2^-24 |ref| (its final conversion) + 1e-12 sum |x| (double accumulation of cancelling terms)."""
    from scanpaths_amd import hip
    from scanpaths_amd.functional import check
    dev, L = _dev(), hip.lib()
    x = _cancelling(n, 120)
    xs = x.double().tolist()
    ref_sum, ref_sq, ref_abs = math.fsum(xs), math.fsum(v * v for v in xs), math.fsum(abs(v) for v in xs)
    xd = x.to(dev)
    ws = torch.empty(L.sp_sumsq_workspace(n), dtype=torch.uint8, device=dev)
    out_f, out_d = torch.full((1,), float("nan"), device=dev), torch.full((1,), float("nan"), dtype=torch.float64, device=dev)
    check(L.sp_sum(hip.ptr(xd), n, hip.ptr(out_f), hip.ptr(ws), hip.stream()), "sp_sum")
    check(L.sp_sumsq(hip.ptr(xd), n, hip.ptr(out_d), hip.ptr(ws), hip.stream()), "sp_sumsq")
    e_sum, bar_sum = abs(float(out_f) - ref_sum), 2.0 ** -24 * abs(ref_sum) + 1e-12 * ref_abs
    e_sq, bar_sq = abs(float(out_d) - ref_sq), 1e-12 * ref_sq
    print(f"PARITY sp_sum / sp_sumsq n={n}: worst err/bar {max(e_sum / bar_sum, e_sq / bar_sq):.3f} (sum: err {e_sum:.2e}, bar {bar_sum:.1e}; "
          f"sumsq: err {e_sq:.2e}, bar {bar_sq:.1e})")
    assert e_sum <= bar_sum, (float(out_f), ref_sum)
    assert e_sq <= bar_sq, (float(out_d), ref_sq)


@pytest.mark.parametrize("n", [1, 3, 4096 * 256 + 77])
def test_clip_adam_and_scale_by_through_the_abi(n):
    """clip_adam_kernel (clip_grad_norm_ + Adam with L2 decay, AiR/train.py:116-117, 200-202) against oracle.clip_and_adam in fp64 with gscale
    folded into the gradients: one element, three, beyond the cap of 4096 blocks; {clip off, above the norm, below it} x {wd 0, 5e-5} x
    {gscale 1, 0.25} x {t = 1, t = 1000}.  Elements with g = p = m = v = 0 stay exactly 0.  scale_by_kernel at the same n.
    The ABI takes beta1 / beta2 as floats, so -- like every other operand -- the oracle is given the values the kernel receives: float32(0.999)
    = 0.99900001287, whose 1 - beta2 = 0.00099998713 is 1.3e-5 (relative) away from 0.001.  The kernel is an exact moving average for THAT
    decay (weights beta2 and 1 - beta2 from the same float).  With the oracle on the double 0.999 instead, v at n = 4096 x 256 + 77 (max g^2 =
    2e2) differs by 2.67e-6 of the 2e-6 bar -- the rounding of the hyper-parameter, not of the arithmetic (p and m passed there)."""
    from oracle import scanpath_oracle as O
    from scanpaths_amd import hip
    from scanpaths_amd.functional import check
    dev, L = _dev(), hip.lib()
    w = Worst(f"sp_clip_adam / sp_scale_by n={n}")
    p0, g0, m0 = _rand(n, seed=130), _rand(n, seed=131) * 3, _rand(n, seed=132) * 0.1
    v0 = (_rand(n, seed=133) * 0.1) ** 2 + 1e-4
    zero = slice(1, 2) if n == 3 else slice(1000, 1300) if n > 3 else slice(0, 0)
    for t in (p0, g0, m0, v0):
        t[zero] = 0.0
    gd = g0.to(dev)
    ws = torch.empty(L.sp_sumsq_workspace(n), dtype=torch.uint8, device=dev)
    sumsq = torch.empty(1, dtype=torch.float64, device=dev)
    check(L.sp_sumsq(hip.ptr(gd), n, hip.ptr(sumsq), hip.ptr(ws), hip.stream()), "sp_sumsq")
    lr, b1, b2, eps = 1e-3, float(np.float32(0.9)), float(np.float32(0.999)), 1e-8          # the betas as the float ABI carries them
    for gscale in (1.0, 0.25):
        norm = math.sqrt(math.fsum(v * v for v in g0.double().tolist())) * gscale
        for clip in (0.0, 2.0 * norm, 0.5 * norm):
            for wd in (0.0, 5e-5):
                for t in (1, 1000):
                    tag = f"gscale={gscale} clip={'off' if clip == 0 else 'above' if clip > norm else 'below'} wd={wd} t={t}"
                    ref = {"x": p0.double().clone()}
                    state = {"step": t - 1, "m.x": m0.double().clone(), "v.x": v0.double().clone()}
                    tn = O.clip_and_adam(ref, {"x": g0.double() * gscale}, state, lr=lr, clip=clip, betas=(b1, b2), eps=eps, weight_decay=wd)
                    assert abs(tn - norm) <= 1e-12 * norm
                    pd, md, vd = p0.to(dev), m0.to(dev), v0.to(dev)
                    check(L.sp_clip_adam(hip.ptr(pd), hip.ptr(gd), hip.ptr(md), hip.ptr(vd), n, hip.ptr(sumsq), gscale, clip, lr, b1, b2, eps, wd,
                                         1.0 - b1 ** t, 1.0 - b2 ** t, hip.stream()), "sp_clip_adam")
                    w.close(pd, ref["x"], 2e-6, f"p ({tag})")
                    w.close(md, state["m.x"], 2e-6, f"m ({tag})")
                    w.close(vd, state["v.x"], 2e-6, f"v ({tag})")
                    if n >= 3:
                        assert float(pd[zero].abs().max()) == 0.0 and float(md[zero].abs().max()) == 0.0 and float(vd[zero].abs().max()) == 0.0
    k = torch.tensor([-0.73], device=dev)
    out = torch.full((n,), float("nan"), device=dev)
    check(L.sp_scale_by(hip.ptr(gd), hip.ptr(k), n, hip.ptr(out), hip.stream()), "sp_scale_by")
    w.close(out, g0.double() * k.cpu().double(), 2e-6, "scale_by")
    w.report()


# ====================================================================================================================
# RL log-probabilities
# ====================================================================================================================
@pytest.mark.parametrize("B,T", [(1, 1), (2, 63), (2, 64), (3, 65), (2, 130)])
def test_rl_log_probabilities(B, T):
    """log_action_kernel / log_duration_kernel / rowscale_kernel (LogAction, LogDuration of AiR/models/loss.py:34-45) through
    scanpaths_amd.models.loss: one step, one 64-lane pass less / exactly / plus one, three passes; an all-zero mask row (exact zero value
    and gradients), probabilities of exactly 0 (log(eps))"""
    from scanpaths_amd.models.loss import LogAction, LogDuration
    w = Worst(f"LogAction / LogDuration B={B} T={T}")
    g = np.random.Generator(np.random.PCG64(140 + T))
    p = torch.from_numpy(g.random((B, T)).astype(np.float32))
    mask = torch.from_numpy((g.random((B, T)) < 0.7).astype(np.float32))
    mask[0, 0] = 1.0
    p[0, 0] = 0.0
    if T > 1:
        p[-1, T // 2] = 0.0
        mask[-1, T // 2] = 1.0
    if B > 1:
        mask[1] = 0.0
    d = _rand(B, T, seed=141).abs() * 0.3 + 0.05
    mu, s2 = _rand(B, T, seed=142), _rand(B, T, seed=143).abs() + 0.3
    ga, gdur = _rand(B, seed=144), _rand(B, seed=145)
    eps = 1e-7
    pr, mur, s2r, mk, dd = p.double().requires_grad_(True), mu.double().requires_grad_(True), s2.double().requires_grad_(True), mask.double(), d.double()
    la_r = (torch.log(pr + eps) * mk).sum(-1) / mk.sum()                                                            # loss.py:34-37
    items = torch.log(1 / (dd + eps) * 1 / torch.sqrt(2 * math.pi * s2r)) + (-(torch.log(dd + eps) - mur) ** 2 / (2 * s2r))
    ld_r = (items * mk).sum(-1) / mk.sum()                                                                          # loss.py:39-45
    ((la_r * ga.double()).sum() + (ld_r * gdur.double()).sum()).backward()
    dev = _dev()
    pg, mug, s2g = (t.to(dev).requires_grad_(True) for t in (p, mu, s2))
    la, ld = LogAction(pg, mask.to(dev)), LogDuration(d.to(dev), mug, s2g, mask.to(dev))
    ((la * ga.to(dev)).sum() + (ld * gdur.to(dev)).sum()).backward()
    w.close(la, la_r, 2e-6, "log_action")
    w.close(ld, ld_r, 2e-6, "log_duration")
    w.close(pg.grad, pr.grad, 2e-6, "dp")
    w.close(mug.grad, mur.grad, 2e-6, "dmu")
    w.close(s2g.grad, s2r.grad, 2e-6, "dsigma2")
    if B > 1:
        assert float(la.detach()[1]) == 0.0 and float(ld.detach()[1]) == 0.0
        assert float(pg.grad[1].abs().max()) == 0.0 and float(mug.grad[1].abs().max()) == 0.0 and float(s2g.grad[1].abs().max()) == 0.0
    w.report()
