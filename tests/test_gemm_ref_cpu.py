"""The conditions tests/test_gemm_fp32_gpu.py relies on, checked without a GPU: the restatement of tests/gemm_ref.py against torch's fp64 conv2d and
its autograd, the branches of the three kernels that the case lists reach (from the library's host-only planning functions and the launch arithmetic
of csrc/conv_igemm.hip), that the bar can see ONE lost k, and that relu cases clip a fair share of their outputs."""
import functools

import pytest
import torch
import torch.nn.functional as TF

import gemm_ref as R
import parity as P


@functools.lru_cache(maxsize=None)
def _problems(group):
    if group == "igemm":
        return [R.IgemmProblem(c) for c in R.igemm_gemm_cases() + R.igemm_conv_cases()]
    if group == "skinny":
        return [R.SkinnyProblem(c) for c in R.skinny_cases()]
    hip, L = P.abi()
    ps = [R.WgradProblem(c) for c in R.wgrad_cases()]
    for p in ps:
        p.splits = R.wgrad_splits(L, p.desc(hip), p.c.Co, p.ldo)[0]
        p.chain = R.chain_wgrad(p.M, p.splits)
    return ps


# ---- the restatement is torch's conv and its autograd ---------------------------------------------------------------
def _nchw(t):
    return t.permute(0, 3, 1, 2)


@pytest.mark.parametrize("case", R.igemm_conv_cases(), ids=lambda c: c.name)
def test_igemm_restatement_is_torchs_conv_and_its_input_gradient(case):
    c, p = case, R.IgemmProblem(case)
    got = R.contract(p.A, p.B)[0]
    x = p.X.live(p.X.flat)[0].double()
    w = p.W.live(p.W.flat)[0].double()
    if c.mode == 0:
        wt = w.reshape(c.Nout, c.KH, c.KW, c.Kc).permute(0, 3, 1, 2)
        ref = TF.conv2d(_nchw(x.reshape(c.N_img, c.Hi, c.Wi, c.Kc)), wt, None, c.stride, c.pad, c.dil)
        assert ref.shape[2:] == (c.Ho, c.Wo)
    else:
        wt = w.reshape(c.Kc, c.KH, c.KW, c.Nout).permute(0, 3, 1, 2)                                      # conv weight [out = c][in = n][ky][kx]
        xin = torch.zeros(c.N_img, c.Nout, c.Ho, c.Wo, dtype=torch.float64, requires_grad=True)
        y = TF.conv2d(xin, wt, None, c.stride, c.pad, c.dil)
        assert y.shape == (c.N_img, c.Kc, c.Hi, c.Wi), (y.shape, c)
        ref, = torch.autograd.grad(y, xin, _nchw(x.reshape(c.N_img, c.Hi, c.Wi, c.Kc)))
    ref = ref.permute(0, 2, 3, 1).reshape(p.M, c.Nout)
    assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


@pytest.mark.parametrize("case", [c for c in R.wgrad_cases() if c.KH > 1], ids=lambda c: c.name)
def test_wgrad_restatement_is_torchs_weight_gradient(case):
    c, p = case, R.WgradProblem(case)
    got = R.contract(p.A, p.B)[0]
    x = p.X.live(p.X.flat)[0].double().reshape(c.N_img, c.Hi, c.Wi, c.Ci)
    dy = p.dY.live(p.dY.flat)[0].double().reshape(c.N_img, c.Ho, c.Wo, c.Co)
    w = torch.zeros(c.Co, c.Ci, c.KH, c.KW, dtype=torch.float64, requires_grad=True)
    y = TF.conv2d(_nchw(x), w, None, c.stride, c.pad, c.dil)
    assert y.shape[2:] == (c.Ho, c.Wo)
    ref, = torch.autograd.grad(y, w, _nchw(dy))
    ref = ref.permute(0, 2, 3, 1).reshape(c.Co, p.Ntot)
    assert (got - ref).abs().max().item() <= 1e-12 * max(1.0, ref.abs().max().item())


def test_epilogue_restatement():
    a, b = P.randn(2, 3, 5, seed=1), P.randn(1, 5, 4, seed=2)
    bias, out0 = P.randn(4, seed=3), P.randn(2, 3, 4, seed=4)
    ref, S = R.reference(a, b, -0.5, bias, out0, True)
    want = torch.relu(-0.5 * torch.matmul(a.double(), b.double()) + bias.double() + out0.double())
    assert torch.equal(ref, want)
    assert (S >= want.abs() - 1e-12).all()                     # S bounds every output it scales the bar of
    assert torch.equal(R.reference(a, b, 1.0, drop=4)[0], torch.matmul(a.double()[..., :4], b.double()[:, :4]))


# ---- the lists reach the branches they were written for ----------------------------------------------------------------
def test_plans_of_gemm_ref_are_the_librarys():
    """skinny_plan against sp_gemm_skinny_workspace for every case, and sp_gemm_skinny_applies = 1 for every case"""
    hip, L = P.abi()
    for p in _problems("skinny"):
        c = p.c
        want = p.nsplit * c.M * c.N * 4 if p.nsplit > 1 else 0
        assert L.sp_gemm_skinny_workspace(c.M, c.N, c.K, c.layout) == want, c
        assert L.sp_gemm_skinny_applies(c.M, c.N, c.K, p.lda, p.ldb, p.ldc, c.layout) == 1, c


def test_skinny_cases_reach_both_epilogues_and_a_16k_last_slice():
    for layout in (0, 1):
        ps = [p for p in _problems("skinny") if p.c.layout == layout]
        assert any(p.nsplit == 1 for p in ps) and any(p.nsplit >= 2 for p in ps)
        assert any(p.nsplit >= 2 and p.c.K - (p.nsplit - 1) * R.skinny_plan(p.c.N, p.c.K, layout)[2] == 16 for p in ps)       # three idle waves
        assert any(p.c.K < 64 for p in ps) and any(p.c.M < 4 for p in ps) and any(p.c.M % 16 and p.c.M % 4 for p in ps)
        for name in ("one-slice", "slices"):                                      # every epilogue combination on the path its name says
            es = [p for p in ps if p.c.name.endswith(name) and "alpha" in p.c.name]
            assert len(es) == 8 and all((p.nsplit == 1) == (name == "one-slice") for p in es)
        assert {p.c.M for p in ps} >= set(R.SK_M) and {p.c.K for p in ps} >= set(R.SK_K) and {p.c.N for p in ps} >= set(R.SK_N[layout])
    off = [p for p in _problems("skinny") if p.c.c_offset]
    assert off and all(p.nsplit == 1 and p.c.layout == 0 and p.ldc == p.c.N + 1 for p in off)


def test_skinny_refusal_table_agrees_with_applies():
    hip, L = P.abi()
    for r in R.skinny_refusals():
        assert L.sp_gemm_skinny_applies(r.M, r.N, r.K, r.K + r.lda_pad, (r.K if r.layout == 0 else r.N) + r.ldb_pad, r.N + r.ldc_pad,
                                        r.layout) == r.applies, r
        if r.offWs != 0:                                                          # the workspace rows are rows in which slices are used
            assert L.sp_gemm_skinny_workspace(r.M, r.N, r.K, r.layout) > 0, r
        if "slices" in r.name:
            assert R.skinny_plan(r.N, r.K, r.layout)[1] > 1, r


def test_wgrad_cases_reach_direct_and_slab_paths():
    ps = _problems("wgrad")
    for beta in (0, 1):
        for alpha in (1.0, -0.5):
            assert any(p.splits == 1 and p.c.beta == beta and p.c.alpha == alpha for p in ps)
            assert any(p.splits > 1 and p.c.beta == beta and p.c.alpha == alpha for p in ps)
    assert any(p.splits > 1 and p.c.KH > 1 for p in ps)
    assert all(p.splits == 1 for p in ps if p.c.nbatch > 1)
    gemm = [p for p in ps if p.c.KH == 1]
    assert {p.M for p in gemm} >= set(R.WG_ROWS) and {p.c.Co for p in gemm} >= set(R.WG_CO) and {p.c.Ci for p in gemm} >= set(R.WG_CI)
    assert any(p.M % 32 == 1 and p.splits == 1 for p in ps)                       # a last K-tile of one row
    assert any(p.c.Ci == 4 and p.c.KH > 1 and p.Ntot < 128 for p in ps)           # a column tile across taps


def test_wgrad_plan_never_leaves_a_split_empty():
    """rows_per_split is rounded up to 32 rows, so a plan could leave its last split without a row (the kernel would then store a slab of zeros:
    `if (nkt > 0)`).  Up to 20000 rows, at 1, 2 and 4 output tiles, no split count the plan chooses does: it keeps >= 256 rows per split
    (smax = M / 256), and rounding up to 32 moves a boundary by < 32 rows per split.  Were one found, its row count would belong in WG_ROWS."""
    hip, L = P.abi()
    assert R.empty_split_rows(L, hip) == []


def test_igemm_cases_reach_both_tiles_modes_folds_and_remainders():
    gemm = [R.IgemmProblem(c) for c in R.igemm_gemm_cases()]
    for mode in (0, 1):
        for narrow in (True, False):
            ps = [p for p in gemm if p.c.mode == mode and (p.c.Nout <= 64) == narrow]
            plans = [R.igemm_plan(p.c.Kc, 1, p.c.ksplit, p.c.nbatch, mode) for p in ps]
            assert any(kps >= 8 for _, kps, _ in plans)                            # the fold inside the loop (kt = 7)
            assert any(kps >= 16 for _, kps, _ in plans)                           # ... and at kt = 15
            assert any(kps % 8 for _, kps, _ in plans if kps > 8)                  # a remainder after a fold
            assert any(kps == 8 for _, kps, _ in plans)                            # and none
            assert any(p.c.Kc % 32 for p in ps)                                    # kvalid / k < Ktot
            assert {ks for _, _, ks in plans} >= {1, 2, 3, 4, 7}
            assert any(ks > 1 and nkt % kps for nkt, kps, ks in plans)             # a shorter last split
            assert any(p.c.ksplit > ks > 1 for p, (_, _, ks) in zip(ps, plans))    # a recomputed split count
            assert any(p.c.nbatch > 1 and p.c.shared_w for p in ps) and any(p.c.nbatch > 1 and not p.c.shared_w for p in ps)
            assert {p.M for p in ps} >= set(R.IG_M) and {p.c.Kc for p in ps} >= set(R.IG_KC)
            for tag in ("direct", "ksplit3"):
                es = [p for p in ps if p.c.name.endswith(tag) and "bias" in p.c.name]
                assert len({(p.c.bias, p.c.beta, p.c.relu) for p in es}) == 8 and all(p.c.alpha == -0.5 for p in es)
        assert {p.c.Nout for p in gemm if p.c.mode == mode} >= set(R.IG_NOUT[mode])
    conv = [R.IgemmProblem(c) for c in R.igemm_conv_cases()]
    small = [p for p in conv if p.c.Kc == 4]
    assert {(p.c.KH, p.c.Nout) for p in small} == {(7, 64), (7, 96), (3, 64), (3, 96)}
    assert all((p.c.KH * p.c.KW) % 8 == 1 for p in small)                          # one tap in the last tap tile
    for mode in (0, 1):
        assert any(p.c.mode == mode and p.c.stride == 2 and p.c.dil == 2 for p in conv)
        assert any(p.c.mode == mode and p.c.N_img == 3 and (p.c.Ho * p.c.Wo) % 128 for p in conv)        # an M-tile across images


# ---- the bar has teeth, relu cases clip --------------------------------------------------------------------------------
@pytest.mark.parametrize("group", ["igemm", "skinny", "wgrad"])
def test_the_bar_sees_one_lost_k(group):
    """the fp64 reference with ONE k left out (the last that any output reads) misses the bar somewhere, in every case with K <= 4096"""
    n = 0
    for p in _problems(group):
        if p.K > 4096:
            continue
        ref, S = p.reference()
        broken, _ = p.reference(drop=R.last_live_k(p.A))
        assert ((broken - ref).abs() > P.bar(S, p.chain)).any(), (group, p.c.name, p.chain)
        n += 1
    assert n > 20


@pytest.mark.parametrize("group", ["igemm", "skinny"])
def test_relu_cases_clip_between_a_fifth_and_four_fifths(group):
    n = 0
    for p in _problems(group):
        if p.c.relu:
            share = (p.reference()[0] == 0).double().mean().item()
            assert 0.2 <= share <= 0.8, (p.c.name, share)
            n += 1
    assert n >= 8


def test_chains_are_the_documented_counts():
    assert R.chain_igemm(36, 1) == 32 * 2 + 1 + 0 + 3 + 1
    assert R.chain_igemm(544, 1) == 256 + 3 + 0 + 3 + 1
    assert R.chain_igemm(224, 1, ksplit=5) == 64 + 1 + 4 + 3 + 1
    assert R.chain_igemm(224, 1, ksplit=5, nbatch=3) == R.chain_igemm(224, 1)
    assert R.chain_igemm(4, 49) == 32 * 7 + 1 + 3 + 1
    assert R.chain_skinny(16, 1040, 0) == 16 * 2 + 3 + 8 + 2 + 1
    assert R.chain_skinny(4112, 128, 0) == 16 * 2 + 3 + 0 + 2 + 1
    assert R.chain_wgrad(2049, 8) == 32 * 8 + 2 + 8 + 2 + 1
    assert R.chain_wgrad(33, 1) == 64 + 1 + 0 + 2 + 1
