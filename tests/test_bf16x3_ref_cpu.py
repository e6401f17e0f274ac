"""Holds tests/bf16x3_ref.py -- the reference side of tests/test_conv_bf16x3_gpu.py -- to its claims, on the CPU: the splitter against torch's
bf16 conversion, exact decode, both layouts against a naive loop, R_planes against a naive six-product loop, R_true against torch's fp64 conv and
its autograd, the representation bound, the lattice claims, the split plan at its switch points, and the CPU re-run of w3_kernel's pixel advance
(the parent's one-`if` rule goes wrong on maps of fewer than 16 pixels; the fixed rule is right everywhere)."""
import numpy as np
import pytest
import torch

import bf16x3_ref as R


def test_splitter_is_torch_bf16_rounding_on_exact_residuals():
    x = R.wide(1 << 16, 1)
    x[:8] = [0.0, -0.0, 1.0, 1.0 + 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -23, 3.0 + 2.0 ** -7, -(2.0 - 2.0 ** -9), 2.0 ** -100]      # ties to even among them
    t = torch.from_numpy(x)
    got = R.split3(x)
    x1 = t.to(torch.bfloat16)
    r1 = t - x1.float()
    x2 = r1.to(torch.bfloat16)
    r2 = r1 - x2.float()
    x3 = r2.to(torch.bfloat16)
    for mine, theirs in zip(got, (x1, x2, x3)):
        assert (mine.view(np.int16) == theirs.view(torch.int16).numpy()).all()
    # the residuals are exact in fp32: the fp64 differences round to themselves
    assert (r1.double() == t.double() - x1.double()).all() and (r2.double() == r1.double() - x2.double()).all()


def test_three_planes_decode_exactly():
    """2^20 normal values across 2^+-30: x1 + x2 + x3 == x, residual 0"""
    x = R.wide(1 << 20, 2)
    assert (np.abs(x) >= 2.0 ** -100).all()
    assert (R.decode3(*R.split3(x)) == x.astype(np.float64)).all()
    g = R.gauss((1 << 16,), 3)
    assert (R.decode3(*R.split3(g)) == g.astype(np.float64)).all()


def test_inf_and_nan_give_value_nan_nan():
    x = np.array([np.inf, -np.inf, np.nan], np.float32)
    x1, x2, x3 = (R.bf16_value(p) for p in R.split3(x))
    assert x1[0] == np.inf and x1[1] == -np.inf and np.isnan(x1[2])
    assert np.isnan(x2).all() and np.isnan(x3).all()
    # a finite value that rounds past the largest bf16 (|x| >= 2^128 - 2^119): (inf, -inf, NaN) -- a NaN plane again, never a finite wrong value
    big = [R.bf16_value(p)[0] for p in R.split3(np.array([3.4e38], np.float32))]
    assert big[0] == np.inf and big[1] == -np.inf and np.isnan(big[2])


def test_layouts_against_a_naive_loop():
    rows, K = 3, 48
    x = R.gauss((rows, K), 4)
    buf = R.split3_bf16(x)
    assert buf.size == 3 * rows * K + 32 and (buf[-32:] == 0).all()
    planes = R.split3(x)
    for r in range(rows):
        for k in range(K):
            for pl in range(3):
                assert buf[((r * (K // 16) + k // 16) * 3 + pl) * 16 + k % 16] == planes[pl][r, k]
    for got, want in zip(R.unpack3(buf, rows, K), planes):
        assert (got == R.bf16_value(want)).all()
    Co, taps, Ci = 16, 3, 5
    w = R.gauss((Co, taps, Ci), 5)
    buf = R.split3_bf16_wT(w)
    assert buf.size == 3 * w.size + 32 and (buf[-32:] == 0).all()
    planes = R.split3(w)
    for co in range(Co):
        for tap in range(taps):
            for ci in range(Ci):
                k = tap * Co + co
                for pl in range(3):
                    assert buf[((ci * (taps * Co // 16) + k // 16) * 3 + pl) * 16 + k % 16] == planes[pl][co, tap, ci]


@pytest.mark.parametrize("kind", ["gauss", "lattice"])
def test_planes_contraction_is_the_six_products(kind):
    for mode in (0, 1):
        p = R.B3Problem(R._bc(f"naive-mode{mode}", 1, 2, 3, 16, 3, 3, 1, 1, 1, mode, bias=False), kind)
        want = p.alpha * R.six_naive([a[0] for a in p.Ap], [b[0] for b in p.Bp])
        assert (p.planes()[0][0] - want).abs().max() <= 1e-13 * p.planes()[1].max()
        # and NOT with the dropped products: on Gaussian data a2 b3 + a3 b2 + a3 b3 is visible in fp64
        if kind == "gauss":
            full = p.alpha * torch.matmul(sum(p.Ap), sum(p.Bp))
            assert (full - p.planes()[0]).abs().max() > 0
            assert (full - p.true()).abs().max() <= 1e-13 * p.planes()[1].max()          # all nine products are the true product: exact decode
    w = R.W3Problem(R._wc("naive-wgrad", 2, 2, 3, 128, 16, 3, 1, 1, 1), kind)
    want = w.alpha * R.six_naive([a[0][:2] for a in w.Ap], [b[0][:, :5] for b in w.Bp])
    assert (w.planes()[0][0, :2, :5] - want).abs().max() <= 1e-13 * w.planes()[1].max()


CONVS = [(3, 1, 1, 1), (3, 2, 1, 1), (3, 1, 2, 2), (3, 2, 2, 2), (7, 2, 3, 1), (1, 1, 0, 1)]


@pytest.mark.parametrize("k,stride,pad,dil", CONVS)
def test_true_contraction_is_torch_conv_and_its_autograd(k, stride, pad, dil):
    N, H, W, C, Co = 2, 9, 13, 16, 20
    f = R._bc("fwd", N, H, W, C, Co, k, stride, pad, dil, 0, bias=True, relu=True, alpha=1.0)
    p = R.B3Problem(f, "gauss")
    x = torch.from_numpy(p.x).double().reshape(N, H, W, C).permute(0, 3, 1, 2).requires_grad_()
    w = torch.from_numpy(p.w).double().reshape(Co, k, k, C).permute(0, 3, 1, 2).requires_grad_()
    y = torch.nn.functional.conv2d(x, w, p.bias.double(), stride=stride, padding=pad, dilation=dil)
    want = torch.relu(y).permute(0, 2, 3, 1).reshape(1, p.M, Co)
    assert (p.true() - want).abs().max() <= 1e-12
    # data gradient: the launch's X is dY [N, h, w, Co'], Kc = the conv's Co; its Nout = the conv's Ci
    Cg = 16
    b = R.B3Problem(R._bc("bwd", N, H, W, Cg, 12, k, stride, pad, dil, 1, bias=False, alpha=1.0), "gauss")
    xin = torch.zeros(N, 12, H, W, dtype=torch.float64, requires_grad=True)
    wc = torch.from_numpy(b.w).double().reshape(Cg, k, k, 12).permute(0, 3, 1, 2)          # [Co][Ci][kh][kw]
    dy = torch.from_numpy(b.x).double().reshape(N, b.c.Hi, b.c.Wi, Cg).permute(0, 3, 1, 2)
    torch.nn.functional.conv2d(xin, wc, None, stride=stride, padding=pad, dilation=dil).backward(dy)
    assert (b.true() - xin.grad.permute(0, 2, 3, 1).reshape(1, b.M, 12)).abs().max() <= 1e-12
    # weight gradient
    g = R.W3Problem(R._wc("wgrad", N, H, W, 128, 16, k, stride, pad, dil, alpha=1.0), "gauss")
    xi = torch.from_numpy(g.x).double().reshape(N, H, W, 128).permute(0, 3, 1, 2)
    ww = torch.zeros(16, 128, k, k, dtype=torch.float64, requires_grad=True)
    dyw = torch.from_numpy(g.dy).double().reshape(N, g.c.Ho, g.c.Wo, 16).permute(0, 3, 1, 2)
    torch.nn.functional.conv2d(xi, ww, None, stride=stride, padding=pad, dilation=dil).backward(dyw)
    assert (g.true() - ww.grad.permute(0, 2, 3, 1).reshape(1, 16, g.Ntot)).abs().max() <= 1e-11


@pytest.mark.parametrize("kind", ["gauss", "heavy"])
def test_rep_bound_holds(kind):
    for case in (R._bg("rep-gemm", 257, 272, 129, 0), R._bc("rep-conv", 3, 5, 7, 48, 60, 3, 1, 1, 1, 1, relu=True, beta=1)):
        p = R.B3Problem(case, kind)
        d = (p.planes()[0] - p.true()).abs()
        assert (d <= p.rep_bar()).all()
        assert d.max() > 0 or kind == "heavy"
    w = R.W3Problem(R._wg("rep-wgrad", 1023, 48, 128, beta=1), kind)
    assert ((w.planes()[0] - w.true()).abs() <= w.rep_bar()).all()


def test_lattice_claims():
    """the splitter returns the intended planes (asserted inside lattice_values), every product is on the 2^-16 lattice, S stays within 2^24
    units, every K-tile reaches some output, and all three planes are live on both sides"""
    for p in [R.B3Problem(c, "lattice") for c in (R._bg("l-nkt1", 257, 16, 129, 0), R._bg("l-nkt33", 257, 528, 129, 1),
                                                  R._bc("l-7x7", 1, 9, 13, 16, 64, 7, 2, 3, 1, 0), R._bg("l-super", 1024, 16, 1024, 0, bias=False))] + \
             [R.W3Problem(c, "lattice") for c in (R._wg("l-rows33", 33, 48, 128), R.W3_CAP, R._wc("l-map-2x2", 18, 2, 2, 128, 16, 1, 1, 0, 1))]:
        ref, S = p.planes()
        assert p.exact_span() <= 2.0 ** 24
        unit = abs(p.alpha) * R.LATTICE_UNIT
        assert (torch.round(ref / unit) * unit == ref).all()
        assert ref.float().double().eq(ref).all()                       # the exact result is an fp32 number
        assert p.live_tiles() >= (1.0 if isinstance(p, R.B3Problem) and p.c.KH == 1 else 0.9), (p.c.name, p.live_tiles())
        assert all((a != 0).any() for a in p.Ap) and all((b != 0).any() for b in p.Bp)
        assert (ref != 0).any()
    # all three planes live limits K: dense full values at K = 16 already use 16 x 25 of the 256 units
    x, planes = R.lattice_values(np.ones((1, 16), bool), 7, full_share=1.0)
    assert float(np.abs(planes[0]).sum()) * 5.0 > 256


def test_split_plan_at_its_switch_points():
    S = R.w3_splits
    assert [S(M, 16, 128) for M in (1, 1023, 1024, 1535, 1536, 2047, 2048, 32767, 32768, 1 << 20)] == [1, 1, 2, 2, 3, 3, 4, 63, 64, 64]
    assert S(4096, 272, 128) == 8 and S(1 << 20, 272, 1152) == 64 and S(1 << 20, 2048, 4608) == 8          # cdiv(2048, tiles) limits
    assert R.rows_per_split(1024, 2) == 512 and R.rows_per_split(1025, 2) == 528 and R.rows_per_split(1040, 2) == 528
    assert R.rows_per_split(1537, 3) == 528 and R.rows_per_split(32768, 64) == 512
    assert R.w3_workspace(1023, 16, 128, 132) == 0 and R.w3_workspace(1024, 16, 128, 132) == 2 * 16 * 132 * 4
    assert R.chain_w3(1024, 2) > R.chain_w3(512, 1) and R.chain_b3(16, 1) < R.chain_b3(32, 1) < R.chain_b3(256, 1) == R.chain_b3(272, 1) < R.chain_b3(512, 1)
    assert R.chain_b3(16, 1) == (2 * 96 + 1 + 3) + 1 + 1          # 196 roundings, one for the (1 + u)^n expansion, one for the reference


WRONG = [(1, 1), (2, 2), (3, 3), (3, 5), (1, 15), (15, 1), (7, 2)]
RIGHT = [(4, 4), (2, 8), (3, 6), (1, 16), (16, 1), (5, 5)]


def test_pixel_advance_old_rule_fails_below_16_pixels_fixed_rule_never():
    for (Ho, Wo) in WRONG + RIGHT:
        for m_begin in (0, 512, 528):
            true = R.w3_walk_true(Ho, Wo, 40, m_begin)
            old = R.w3_walk(Ho, Wo, 40, m_begin, fixed=False)
            new = R.w3_walk(Ho, Wo, 40, m_begin, fixed=True)
            assert (new == true).all(), (Ho, Wo, m_begin)
            assert (old[0] == true[0]).all()
            if (Ho, Wo) in WRONG:
                assert (old[1:] != true[1:]).any(), (Ho, Wo)
                assert (old[..., 0] <= true[..., 0]).all()               # the wrong image index never runs ahead: the addresses stay inside the operand
            else:
                assert (old == true).all(), (Ho, Wo)
    for Ho in range(1, 21):
        for Wo in range(1, 21):
            assert (R.w3_walk(Ho, Wo, 12, 7, fixed=True) == R.w3_walk_true(Ho, Wo, 12, 7)).all(), (Ho, Wo)
            if Ho * Wo >= 16:
                assert (R.w3_walk(Ho, Wo, 12, 7, fixed=False) == R.w3_walk_true(Ho, Wo, 12, 7)).all(), (Ho, Wo)
