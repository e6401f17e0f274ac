"""The reference of the 2xfp16 kernels (tests/f16x2_ref.py) held to what it claims, without a GPU: the splitter emulation against the header's format
written out index by index, R_true's gathers against torch's fp64 conv2d and autograd at 1e-12, R_planes against R_true inside the derived
representation bound for every case, exactness of the lattice data (the guaranteed condition per case and its brute-force check), the plans
against the library's host-side queries, and the teeth of the bar."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import f16x2_ref as R
import parity as P

F32, F16 = np.float32, np.float16
KINDS = ("gauss", "lattice")
LISTS = {"h2_gemm": R.h2_gemm_cases, "h2_conv": R.h2_conv_cases, "h2_stats": R.h2_stats_cases, "h2_x1": R.h2_x1_cases, "h2_batched": R.h2_batched_cases,
         "hw": R.hw_cases, "hw_x1": R.hw_x1_cases, "hw_batched": R.hw_batched_cases}


@functools.lru_cache(maxsize=None)
def _problem(group, case, kind):
    return (R.H2Problem if group.startswith("h2") else R.HWProblem)(case, kind)


def _problems(group, kind):
    return [_problem(group, c, kind) for c in LISTS[group]()]


# ---- splitters -----------------------------------------------------------------------------------------------------------
def test_scale_of_is_the_headers_rule():
    for a, want in ((0.0, 1.0), (float("inf"), 1.0), (float("nan"), 1.0), (-1.0, 1.0), (8192.0, 1.0), (16383.0, 1.0), (16384.0, 0.5),
                    (1.0, 8192.0), (0.75, 16384.0), (1e-38, 2.0 ** 126), (2.0 ** -149, 2.0 ** 126), (3e38, 2.0 ** -114), (2.0 ** -100, 2.0 ** 113)):
        assert float(R.scale_of(a)) == want, (a, float(R.scale_of(a)), want)
    g = np.random.Generator(np.random.PCG64(1))
    for a in np.exp(g.uniform(-60, 60, 500)).astype(F32):
        assert 8192.0 <= float(a) * float(R.scale_of(a)) < 16384.0


def test_split2_residual_and_storage():
    g = np.random.Generator(np.random.PCG64(2))
    x = (g.standard_normal(4096) * np.exp(g.uniform(-12, 0, 4096))).astype(F32)
    planes, s = R.split2_f16(x)
    assert planes.size == 2 * x.size + 32 and not planes[-32:].any()                       # the 64-byte zero block
    x1, x2 = R.unpack(planes, 1, x.size)
    xs = x.astype(np.float64) * float(s)
    assert 8192 <= np.abs(xs).max() < 16384
    assert (np.abs(xs - x1[0] - x2[0]) <= 2.0 ** -22 * np.abs(xs) + 2.0 ** -25).all()
    assert (np.abs(x2[0]) <= 2.0 ** -11 * (1 + 2.0 ** -11) * np.abs(xs) + 2.0 ** -24).all()
    # [row][K / 16][plane][16], written out
    a, b = R.split2(x, s)
    for k in (0, 15, 16, 31, 4095):
        assert planes[(k // 16) * 32 + k % 16] == a.view(np.uint16)[k] and planes[(k // 16) * 32 + 16 + k % 16] == b.view(np.uint16)[k]
    # wider rows: the pad columns are NaNs and unpack skips them
    p = R.pack(a.reshape(128, 32), b.reshape(128, 32), 48)
    assert p.size == 2 * 128 * 48 + 32 and (R.unpack(p, 128, 32, 48)[0] == x1.reshape(128, 32)).all()
    assert (p[:-32].reshape(128, 3, 2, 16)[:, 2] == R.F16_NAN).all()
    # have_amax: a bound 7 x the maximum lowers the scale, the planes stay a split of x s
    p7, s7 = R.split2_f16(x, bound=7 * np.abs(x).max())
    assert float(s7) in (float(s) / 4, float(s) / 8) and R.split2_f16(x, bound=np.abs(x).max())[1] == s


def test_entry_point_layouts_index_by_index():
    g = np.random.Generator(np.random.PCG64(3))
    Co, taps, Ci = 16, 3, 8
    w = g.standard_normal((Co, taps, Ci)).astype(F32)
    planes, s = R.split2_f16_wT(w)
    x1, x2 = R.unpack(planes, Ci, taps * Co)
    for co, tap, ci in ((0, 0, 0), (15, 2, 7), (3, 1, 5)):
        a, b = R.split2(w[co, tap, ci], s)
        assert x1[ci, tap * Co + co] == float(a) and x2[ci, tap * Co + co] == float(b)
    # rows with absorb: w[r][tap][c] / absorb[c], one scale per row
    Kc = 16
    wr = g.standard_normal((3, 2 * Kc)).astype(F32)
    wr[1] = 0                                                                                  # a row of zeros: scale 1
    absorb = (2.0 ** g.integers(-3, 4, Kc)).astype(F32)
    absorb[5] = 2.0 ** -30
    planes, sr = R.split2_f16_rows(wr, Kc, absorb)
    assert sr[1] == 1.0 and sr.shape == (3,)
    x1, x2 = R.unpack(planes, 3, 2 * Kc)
    for r, k in ((0, 5), (2, 21), (2, 31)):
        v = F32(wr[r, k] / absorb[k % Kc])
        a, b = R.split2(v, sr[r])
        assert x1[r, k] == float(a) and x2[r, k] == float(b)
    assert 8192 <= np.abs(x1[2] + x2[2]).max() < 16384.5
    # wT_rows: rows (item, ci), k = (tap, co), value w / absorb[co]
    w4 = g.standard_normal((2, Co, taps, Ci)).astype(F32)
    w4[1, :, :, 3] = 0
    ab = (2.0 ** g.integers(-3, 4, Co)).astype(F32)
    planes, s4 = R.split2_f16_wT_rows(w4, ab)
    assert s4.shape == (2 * Ci,) and s4[Ci + 3] == 1.0
    x1, x2 = R.unpack(planes, 2 * Ci, taps * Co)
    for it, co, tap, ci in ((0, 0, 0, 0), (1, 15, 2, 7), (1, 4, 1, 2)):
        a, b = R.split2(F32(w4[it, co, tap, ci] * (F32(1) / ab[co])), s4[it * Ci + ci])
        assert x1[it * Ci + ci, tap * Co + co] == float(a) and x2[it * Ci + ci, tap * Co + co] == float(b)
    # cols: one scale per channel, 2^100 for a dead one
    x = g.standard_normal((5, 16)).astype(F32) * (2.0 ** g.integers(-8, 8, 16)).astype(F32)
    x[:, 7] = 0
    planes, sc = R.split2_f16_cols(x)
    assert sc[7] == F32(2.0 ** 100) and all(8192 <= np.abs(x[:, c]).max() * sc[c] < 16384 for c in range(16) if c != 7)
    x1, x2 = R.unpack(planes, 5, 16)
    assert (x1[:, 7] == 0).all() and np.allclose(x1 + x2, x.astype(np.float64) * sc.astype(np.float64), rtol=2.0 ** -21, atol=2.0 ** -24)
    assert R.colamax_blocks(5, 16) == 1 and R.colamax_blocks(512 * 64 * 4 + 1, 16) == 512 and R.colamax_blocks(9, 1040) == 3


# ---- lattice data -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rich", (False, True))
def test_lattice_planes_are_h_and_l(rich):
    for axes, shape in (((), (3, 40, 32)), ((0, 1), (2, 5, 64)), ((2,), (1, 33, 16))):
        x, h, l = R.lattice(shape, axes, 11, rich)
        amax = np.abs(x)
        for a in range(len(shape)):
            if a not in axes:
                amax = amax.max(axis=a, keepdims=True)
        s = R.scales_of(amax)
        assert (x.astype(np.float64) * s == h + l).all() and (amax * s == 8192).all()      # the pin sets the scale: x s is the lattice value
        x1, x2 = R.split2(x, s)
        assert (x1.astype(np.float64) == h).all() and (x2.astype(np.float64) == l).all()
        assert ((l == 0) | (h != 0)).all()


@pytest.mark.parametrize("group", sorted(LISTS))
def test_lattice_cases_are_guaranteed_exact(group):
    """largest possible partial sum / granularity <= 2^24 in every case: then every fp32 summation order, and the epilogue, is exact; and the fp64
    R_planes is itself on the fp32 grid"""
    worst = 0.0
    for p in _problems(group, "lattice"):
        span = p.exact_span()
        worst = max(worst, span)
        assert span <= 2.0 ** 24, (p.c.name, np.log2(span))
        ref, _ = p.planes()
        assert torch.equal(ref.float().double(), ref), p.c.name
        assert torch.equal((ref / torch.from_numpy(p.unit)).round() * torch.from_numpy(p.unit), ref), p.c.name
    print(f"LATTICE {group}: largest span 2^{np.log2(worst):.2f}")


@pytest.mark.parametrize("K,rich", ((256, False), (2592, False), (4096, False), (288, True)))
def test_lattice_condition_brute_force(K, rich):
    """sequential and randomly permuted fp32 sums of the 3 K products of one output element equal the exact sum, partial sum by partial sum"""
    g = np.random.Generator(np.random.PCG64(K))
    for trial in range(20):
        (a, ha, la), (b, hb, lb) = R.lattice((K,), (), 100 + trial, rich), R.lattice((K,), (), 200 + trial, rich)
        prods = np.concatenate([ha * lb, la * hb, ha * hb])
        gran = 1024.0 if rich else 4096.0
        if np.abs(prods).sum() / gran > 2.0 ** 24:
            continue
        for order in (np.arange(3 * K), g.permutation(3 * K)):
            seq = np.cumsum(prods[order].astype(F32), dtype=F32)
            assert (seq.astype(np.float64) == np.cumsum(prods[order])).all()


# ---- R_true is torch's conv and its gradients ---------------------------------------------------------------------------------
def _nchw(x):
    return x.permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", R.h2_conv_cases() + R.h2_stats_cases() + R.h2_x1_cases()[3:], ids=lambda c: c.name)
def test_h2_restatement_is_torchs_conv_and_its_input_gradient(case):
    c, p = case, _problem("h2", case, "gauss")
    got = torch.matmul(p.A, p.B)[0]
    x, w = torch.from_numpy(p.x[0]).double(), torch.from_numpy(p.w[0]).double()
    wt = w.reshape(c.Nout, c.KH, c.KW, c.Kc)                                                   # [n][ky][kx][channel of the launch's X]
    if c.mode == 0:
        ref = TF.conv2d(_nchw(x.reshape(c.N_img, c.Hi, c.Wi, c.Kc)), wt.permute(0, 3, 1, 2), None, c.stride, c.pad, c.dil)
        assert ref.shape[2:] == (c.Ho, c.Wo)
    else:                                                                                      # conv weight [out = Kc channel][in = n][ky][kx]
        xin = torch.zeros(c.N_img, c.Nout, c.Ho, c.Wo, dtype=torch.float64, requires_grad=True)
        y = TF.conv2d(xin, wt.permute(3, 0, 1, 2), None, c.stride, c.pad, c.dil)
        assert y.shape[2:] == (c.Hi, c.Wi)
        ref, = torch.autograd.grad(y, xin, _nchw(x.reshape(c.N_img, c.Hi, c.Wi, c.Kc)))
    ref = ref.permute(0, 2, 3, 1).reshape(p.M, c.Nout)
    assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("case", [c for c in R.hw_cases() + R.hw_x1_cases() if c.KH > 1], ids=lambda c: c.name)
def test_hw_restatement_is_torchs_weight_gradient(case):
    c, p = case, _problem("hw", case, "gauss")
    got = torch.matmul(p.A, p.B)[0]
    x = torch.from_numpy(p.x[0]).double().reshape(c.N_img, c.Hi, c.Wi, c.Ci)
    dy = torch.from_numpy(p.dy[0]).double().reshape(c.N_img, c.Ho, c.Wo, c.Co)
    w = torch.zeros(c.Co, c.Ci, c.KH, c.KW, dtype=torch.float64, requires_grad=True)
    y = TF.conv2d(_nchw(x), w, None, c.stride, c.pad, c.dil)
    assert y.shape[2:] == (c.Ho, c.Wo)
    ref, = torch.autograd.grad(y, w, _nchw(dy))
    ref = ref.permute(0, 2, 3, 1).reshape(c.Co, p.Ntot)
    assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


# ---- representation error -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ("gauss", "heavy", "lattice"))
@pytest.mark.parametrize("group", sorted(LISTS))
def test_planes_are_within_the_representation_bound_of_the_true_product(group, kind):
    worst = (0.0, "")
    for p in _problems(group, kind):
        planes, S = p.planes()
        q =((planes - p.true()).abs() / p.rep_bar()).max().item()
        worst = max(worst, (q, p.c.name))
        assert q <= 1.0, (p.c.name, q)
    print(f"REPRESENTATION {group} {kind}: worst error / bound {worst[0]:.3f} at {worst[1]}")


# ---- plans -----------------------------------------------------------------------------------------------------------------------
def test_split_plans_are_the_librarys():
    hip, L = P.abi()
    for group in ("hw", "hw_x1", "hw_batched"):
        for p in _problems(group, "gauss"):
            want = p.splits * p.c.Co * p.ldo * 4 if p.splits > 1 else 0
            assert L.sp_conv_wgrad_f16x2_workspace(ctypes.byref(R.hw_desc(hip, p))) == want, p.c.name
    g = np.random.Generator(np.random.PCG64(5))
    for _ in range(300):
        M, Co, Ci, taps = int(g.integers(1, 200000)), 16 * int(g.integers(1, 40)), 16 * int(g.integers(1, 40)), int(g.choice([1, 9]))
        k = 1 if taps == 1 else 3
        d = hip.WgradDesc(N_img=1, Hi=M, Wi=1, Ci=Ci, ldx=Ci, Ho=M, Wo=1, Co=Co, ldy=Co, KH=k, KW=k, stride=1, pad=k // 2, dil=1, ldo=taps * Ci, beta=0,
                          alpha=1.0, nbatch=1)
        sp = R.hw_splits(M, Co, taps * Ci)
        assert L.sp_conv_wgrad_f16x2_workspace(ctypes.byref(d)) == (sp * Co * taps * Ci * 4 if sp > 1 else 0), (M, Co, Ci, taps, sp)
    for N, H, W, Ci, Co, k, nseg in ((1, 32, 64, 256, 256, 1, 1), (1, 32, 64, 256, 256, 3, 3), (32, 32, 64, 256, 512, 3, 15), (1, 32, 64, 256, 256, 1, 16),
                                     (3, 64, 64, 128, 256, 3, 2), (1, 32, 20, 256, 256, 1, 1), (1, 32, 64, 256, 128, 1, 1), (1, 32, 64, 256, 256, 1, 17)):
        c = R._wc("multi", N, H, W, Ci, Co, k, 1, k // 2, 1, ldo_pad=4)
        ldo = k * k * Ci + 4
        d = hip.WgradDesc(N_img=N, Hi=H, Wi=W, Ci=Ci, ldx=Ci, Ho=H, Wo=W, Co=Co, ldy=Co, KH=k, KW=k, stride=1, pad=k // 2, dil=1, ldo=ldo, beta=0,
                          alpha=1.0, nbatch=1)
        want = nseg * R.hw2_splits(N * H * W, Co, k * k * Ci, nseg) * Co * ldo * 4 if R.hw2_applies(c, nseg, ldo) else 0
        assert L.sp_conv_wgrad_f16x2_multi_workspace(ctypes.byref(d), nseg) == want, (N, H, W, Ci, Co, k, nseg)


def test_every_build_of_the_product_library_is_named_by_a_case():
    names = {p.build for g in LISTS for p in _problems(g, "gauss")}
    for mode in (0, 1):
        for order in ("tap-major", "cbm", "halo"):
            assert f"h2<mode{mode},nprod3,{order}>" in names, (mode, order)
        assert f"h2<mode{mode},nprod1,tap-major>" in names
    assert {"h2<mode0,nprod3,cbm>+stats", "h2<mode0,nprod3,tap-major>+stats"} <= names
    assert {"hw<nprod3>", "hw<nprod3>+hw_reduce4", "hw<nprod3>+hw_reduce", "hw<nprod3>+batched", "hw<nprod1>", "hw<nprod1>+hw_reduce4",
            "hw<nprod1>+hw_reduce"} <= names, names
    # the shapes written for one build run it, and the ones beside them do not
    for c in R.h2_conv_cases():
        if "halo" in c.name:
            assert R.halo_applies(c) == ("not" not in c.name), c.name
    assert not R.cbm_ok(next(c for c in R.h2_conv_cases() if c.name == "mode1-stride2-dil2-9x13"))
    assert not R.cbm_ok(next(c for c in R.h2_conv_cases() if "49-taps" in c.name))
    assert R.row_nimg(R._hc("x", 64, 4, 64, 32, 32, 3, 1, 1, 1, 1), True) == 64 and R.row_nimg(R._hc("x", 65, 4, 64, 32, 32, 3, 1, 1, 1, 1), True) == 0


def test_case_lists_reach_the_edges_they_were_written_for():
    gemm = R.h2_gemm_cases()
    for mode in (0, 1):
        cs = [c for c in gemm if c.mode == mode]
        assert {c.N_img for c in cs} >= set(R.H2_M) and {c.Nout for c in cs} >= set(R.H2_NOUT) and {c.Kc for c in cs} >= set(R.H2_KC)
        assert {(c.bias, c.beta, c.relu) for c in cs if "stores" in c.name and c.Nout % 4} == {(b, e, r) for b in (False, True) for e in (0, 1) for r in (False, True)}
        assert any(c.sw_rows for c in cs) and any(c.ldx_pad == 16 for c in cs) and any((c.Nout + c.ldc_pad) % 4 for c in cs)
    hw = _problems("hw", "gauss")
    assert {p.M for p in hw} >= set(R.HW_ROWS) and {p.c.Co for p in hw} >= set(R.HW_CO) and {p.c.Ci for p in hw} >= set(R.HW_CI)
    assert any(p.splits > 1 and p.c.KH > 1 for p in hw) and {p.Ntot for p in hw if p.c.KH == 3} >= {144, 288, 432}
    for a in (1.0, -0.5):
        for b in (0, 1):
            assert {p.reducer for p in hw if p.c.alpha == a and p.c.beta == b} >= {None, "hw_reduce4", "hw_reduce"}
    for xv in (False, True):
        for yv in (False, True):
            assert {p.reducer for p in hw if p.c.xvec == xv and p.c.yvec == yv} >= {None, "hw_reduce4", "hw_reduce"}
    assert {(p.ldo, p.Nvalid) for p in (R.HWProblem(c) for c in R.hw_batched_cases())} == {(12, 12), (20, 16)}


def test_chains_are_the_documented_counts():
    c = R._chain
    assert R.chain_h2(32, 1) == c(2 * 96 * 1 + 1 + 5) and R.chain_h2(288, 1) == c(2 * 96 * 8 + 2 + 5) and R.chain_h2(544, 1) == c(2 * 96 * 8 + 3 + 5)
    assert R.chain_h2(32, 9) == c(2 * 96 * 8 + 2 + 5) and R.chain_h2(64, 1, nprod=1) == c(2 * 32 * 2 + 1 + 5)
    assert R.chain_hw(33, 1) == c(2 * 96 * 2 + 1 + 4) and R.chain_hw(2049, 2) == c(2 * 96 * 8 + 5 + 2 + 5)
    assert R.chain_hw2(2048, 1, 3) == c(2 * 96 * 64 + 1 + 2 + 3 + 2)
    assert R._chain(200) == 200 + 1 + 1 and R._chain(100000) == 100000 + 1193 + 1          # n (1 + 2 n 2^-24) rounded up, plus one


# ---- teeth -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", sorted(LISTS))
def test_the_bar_sees_one_lost_k(group):
    """R_planes with the last live k left out misses the derived bar somewhere in every case with K <= 4096; on lattice data it differs in bits"""
    n = 0
    for p in _problems(group, "gauss"):
        if p.K > 4096:
            continue
        ref, S = p.planes()
        broken, _ = p.planes(drop=p.last_live_k())
        assert ((broken - ref).abs() > P.bar(S, p.chain)).any(), (group, p.c.name, p.chain)
        pl = _problem(group, p.c, "lattice")
        assert not torch.equal(pl.planes(drop=pl.last_live_k())[0].float(), pl.planes()[0].float()), p.c.name
        n += 1
    assert n >= 5


@pytest.mark.parametrize("group", sorted(g for g in LISTS if "x1" not in g))
def test_the_bar_sees_one_lost_cross_term(group):
    """R_planes without a1 b2 of ONE 32-k K-tile (the last) misses the bar in every case of at most two K-tiles; which longer cases it still holds
    for is printed.  On lattice data the change is a bit mismatch whatever the length."""
    held, lost = [], []
    for p in _problems(group, "gauss"):
        nkt = p.K // 32
        if nkt < 1:
            continue
        ref, S = p.planes()
        broken, _ = p.planes(cross=nkt - 1)
        seen = bool(((broken - ref).abs() > P.bar(S, p.chain)).any())
        if nkt <= 2:
            assert seen, (group, p.c.name, p.chain)
        else:
            (held if seen else lost).append(f"{p.c.name} ({nkt})")
        pl = _problem(group, p.c, "lattice")
        if (pl.A1[..., -32:] != 0).any() and (pl.B2[:, -32:] != 0).any():
            assert not torch.equal(pl.planes(cross=nkt - 1)[0].float(), pl.planes()[0].float()), p.c.name
    print(f"CROSS-TERM {group}: seen in {len(held)} longer cases, not in {len(lost)}: {', '.join(lost[:12])}")
