"""Plain fp64 restatement of the three fp32 GEMM kernels -- sp_conv_igemm (csrc/conv_igemm.hip), sp_gemm_skinny (csrc/gemm_skinny.hip) and
sp_conv_wgrad (csrc/conv_wgrad.hip) -- the reference side of tests/test_gemm_ref_cpu.py and tests/test_gemm_fp32_gpu.py.  Nothing here touches a GPU.

Every launch is restated as ONE contraction  acc[b][m][n] = sum_k A[b][m][k] B[b][k][n]  in fp64 followed by the epilogue of the ABI:
    igemm   k = (tap, channel): A is the gather of the header's formula written out index by index (im2col / im2col_dgrad), B the weight
    skinny  A, op(B) as given
    wgrad   k = output pixel:   A = dY^T, B = the same gather of X
so that "the last k left out" and the contraction over absolute values S are the same two lines for all of them.  tests/test_gemm_ref_cpu.py
holds the gathers to torch's fp64 conv2d and its autograd at 1e-12.

THE BAR (element-wise, parity.bar):  |got - ref| <= c 2^-24 S + 2^-149,  S =|alpha| (|A| @ |B|) + |bias| + |beta out0|.
fp32 MFMA multiplies exactly and rounds each accumulation once to nearest (unit roundoff u = 2^-24), every other operation of the kernels is one
rounded fp32 operation.  A product that passes through d dependent roundings on its way into an output carries a relative error of at most
(1 + u)^d - 1, so the output's error is at most ((1 + u)^c - 1) S with c the LONGEST such chain of the launch; relu is 1-Lipschitz and changes
nothing.  (1 + u)^c - 1 <= (c + 1) u for every c below 2^12, so each chain_* function below returns its count plus one; that one also covers the
fp64 reference's own error (K 2^-53 S).  The counts are read off the kernels and written next to each function; nothing here was tuned on results."""
from collections import namedtuple

import torch

from parity import Guarded, cdiv, randn, seed_of


# ====================================================================================================================
# chains of dependent roundings
# ====================================================================================================================
def igemm_plan(Kc, taps, ksplit=0, nbatch=1, mode=0):
    """the launch arithmetic of sp_conv_igemm (the lines under `IgemmArgs a;` of csrc/conv_igemm.hip): (nkt, kt_per_split, effective ksplit)"""
    smallc = mode == 0 and Kc == 4 and taps > 1
    nkt = cdiv(taps, 8) if smallc else taps * cdiv(Kc, 32)
    kps, ks = nkt, 1
    if ksplit > 1 and taps == 1 and nbatch == 1 and not smallc:
        kps = cdiv(nkt, ksplit)
        ks = cdiv(nkt, kps)
    return nkt, kps, ks


def chain_igemm(Kc, taps, ksplit=0, nbatch=1, mode=0):
    """A K-tile is 4 x 4 v_mfma_f32_32x32x2_f32 = 32 k, an in-order fmaf chain: 32 roundings per tile, at most CHUNK = 8 tiles before `acc` is
    folded into `tot` and restarted -> 32 min(8, tiles of the split); one add per fold, kt_per_split // 8 folds in the loop and one after it; the
    reducer adds the ksplit slabs one after another (ksplit adds, the first onto 0.f); the epilogue multiplies by alpha, adds bias, adds out:
    3.  Plus one (module docstring)."""
    nkt, kps, ks = igemm_plan(Kc, taps, ksplit, nbatch, mode)
    return 32 * min(8, kps) + (kps // 8 + 1) + (ks if ks > 1 else 0) + 3 + 1


def skinny_plan(N, K, layout):
    """sk_plan of csrc/gemm_skinny.hip: (column workgroups, nsplit, kchunk)"""
    cw = cdiv(N, 16 if layout == 0 else 32)
    want = max(1, min(512 // max(cw, 1), K // 64))
    kchunk = cdiv(cdiv(K, want), 64) * 64
    return cw, cdiv(K, kchunk), kchunk


def chain_skinny(N, K, layout):
    """A wave takes every fourth 16-k block of its slice, 4 v_mfma_f32_16x16x4_f32 = 16 k = 16 roundings per block:
    16 ceil(blocks of the longest slice / 4); wave 0 adds the other three waves' sums: 3; the reducer adds slices 1 .. nsplit - 1 onto slice 0:
    nsplit - 1; alpha and bias: 2.  Plus one."""
    cw, nsplit, kchunk = skinny_plan(N, K, layout)
    blocks = min(kchunk, K) // 16
    return 16 * cdiv(blocks, 4) + 3 + (nsplit - 1) + 2 + 1


def chain_wgrad(rows, splits):
    """A K-tile is 32 pixels = 16 v_mfma_f32_32x32x2_f32 per accumulator = 32 roundings, at most 8 tiles per chunk; folds as in igemm; the
    reducer adds `splits` slabs onto 0.f; alpha and beta * dW: 2.  Plus one."""
    rps = cdiv(cdiv(rows, splits), 32) * 32
    nkt = cdiv(min(rows, rps), 32)
    return 32 * min(8, nkt) + (nkt // 8 + 1) + (splits if splits > 1 else 0) + 2 + 1


def wgrad_splits(lib, desc, Co, ldo):
    """the split count sp_conv_wgrad will use, read from its workspace query"""
    import ctypes
    nbytes = lib.sp_conv_wgrad_workspace(ctypes.byref(desc))
    assert nbytes % (Co * ldo * 4) == 0, (nbytes, Co, ldo)
    return max(1, nbytes // (Co * ldo * 4)), nbytes


# ====================================================================================================================
# the contraction, its epilogue and the bar
# ====================================================================================================================
def contract(A, B, drop=None):
    """[nb, M, K] x [nb or 1, K, N] in fp64; drop: a k index left out"""
    A, B = A.double(), B.double()
    if drop is not None:
        keep = [k for k in range(A.shape[-1]) if k != drop]
        A, B = A[..., keep], B[..., keep, :]
    return torch.matmul(A, B)


def epilogue(acc, alpha, bias=None, out0=None, relu=False):
    """relu?(alpha acc + bias + out0); out0 is given exactly when beta = 1"""
    r = alpha * acc
    if bias is not None:
        r = r + bias.double()
    if out0 is not None:
        r = r + out0.double()
    return r.clamp_min(0.0) if relu else r


def reference(A, B, alpha=1.0, bias=None, out0=None, relu=False, drop=None):
    """(ref, S), both [nb, M, N] fp64"""
    ref = epilogue(contract(A, B, drop), alpha, bias, out0, relu)
    S = epilogue(contract(A.abs(), B.abs()), abs(alpha), None if bias is None else bias.abs(), None if out0 is None else out0.abs())
    return ref, S


def last_live_k(A):
    """the last k whose A column is not zero everywhere (under padding the last tap can lie outside the image for EVERY output pixel: the 1 x 1
    image under 3 x 3 has only its centre tap); the teeth test leaves this one out"""
    live = (A != 0).reshape(-1, A.shape[-1]).any(0).nonzero()
    return int(live[-1])


# ====================================================================================================================
# the gathers of the header (include/scanpaths_amd.h, sp_conv_desc), index by index
# ====================================================================================================================
def im2col(X, KH, KW, stride, pad, dil, Ho, Wo):
    """mode 0 / wgrad: X [N, Hi, Wi, C] -> [N Ho Wo, KH KW C], entry (m, tap, c) = X[b][yo s - p + ky d][xo s - p + kx d][c] or 0 outside"""
    N, Hi, Wi, C = X.shape
    cols = torch.zeros(N, Ho, Wo, KH * KW, C, dtype=X.dtype)
    for ky in range(KH):
        for kx in range(KW):
            for yo in range(Ho):
                iy = yo * stride - pad + ky * dil
                if not 0 <= iy < Hi:
                    continue
                for xo in range(Wo):
                    ix = xo * stride - pad + kx * dil
                    if 0 <= ix < Wi:
                        cols[:, yo, xo, ky * KW + kx] = X[:, iy, ix]
    return cols.reshape(N * Ho * Wo, KH * KW * C)


def im2col_dgrad(dY, KH, KW, stride, pad, dil, Ho, Wo):
    """mode 1: dY [N, Hy, Wy, C] -> [N Ho Wo, KH KW C], entry (m, tap, c) = dY[b][(y + p - ky d) / s][(x + p - kx d) / s][c] where both
    quotients are exact and inside dY, else 0 (the transposed conv)"""
    N, Hy, Wy, C = dY.shape
    cols = torch.zeros(N, Ho, Wo, KH * KW, C, dtype=dY.dtype)
    for ky in range(KH):
        for kx in range(KW):
            for y in range(Ho):
                ty = y + pad - ky * dil
                if ty < 0 or ty % stride or ty // stride >= Hy:
                    continue
                for x in range(Wo):
                    tx = x + pad - kx * dil
                    if tx >= 0 and tx % stride == 0 and tx // stride < Wy:
                        cols[:, y, x, ky * KW + kx] = dY[:, ty // stride, tx // stride]
    return cols.reshape(N * Ho * Wo, KH * KW * C)


def conv_out_size(H, K, stride, pad, dil):
    return (H + 2 * pad - dil * (K - 1) - 1) // stride + 1


# ====================================================================================================================
# igemm cases
# ====================================================================================================================
_IG = namedtuple("IgemmCase", "name N_img Hi Wi Kc Ho Wo Nout KH KW stride pad dil mode alpha bias beta relu nbatch shared_w ksplit")


def _ig(name, M, Kc, Nout, mode, *, alpha=-0.5, bias=True, beta=0, relu=False, nbatch=1, shared_w=True, ksplit=0):
    return _IG(name, M, 1, 1, Kc, 1, 1, Nout, 1, 1, 1, 0, 1, mode, alpha, bias, beta, relu, nbatch, shared_w, ksplit)


IG_M = (1, 127, 128, 129, 257)
IG_KC = (4, 28, 32, 36, 196, 224, 256, 288, 544)           # nkt = 1, 1, 1, 2, 7, 7, 8, 9, 17
IG_NOUT = {0: (1, 63, 64, 65, 129, 192), 1: (4, 60, 64, 68, 132)}
IG_TILE_N = {0: {"narrow": 63, "wide": 65}, 1: {"narrow": 60, "wide": 68}}          # Nout <= 64: the 128 x 64 tile
IG_KSPLITS = (2, 3, 5, 7, 12)                              # at nkt = 7: 2 -> (4, 3); 3 -> (3, 3, 1); 5 -> 4 x 2 less one; 7; 12 -> 7 x 1


def igemm_gemm_cases():
    """taps = 1.  One dimension is swept at a time, each sweep on both tile variants and in both modes; ld = width + pad in every case"""
    cs = []
    for mode in (0, 1):
        for tile, N in IG_TILE_N[mode].items():
            for M in IG_M:
                cs.append(_ig(f"mode{mode}-{tile}-M{M}", M, 36, N, mode))
            for Kc in IG_KC:
                cs.append(_ig(f"mode{mode}-{tile}-Kc{Kc}", 129, Kc, N, mode))
            # epilogue: bias x beta x relu, direct (Kc = 288: one fold and a remainder) and through the split-K reducer
            for bias in (False, True):
                for beta in (0, 1):
                    for relu in (False, True):
                        e = f"bias{int(bias)}beta{beta}relu{int(relu)}"
                        cs.append(_ig(f"mode{mode}-{tile}-{e}-direct", 129, 288, N, mode, bias=bias, beta=beta, relu=relu))
                        cs.append(_ig(f"mode{mode}-{tile}-{e}-ksplit3", 129, 288, N, mode, bias=bias, beta=beta, relu=relu, ksplit=3))
            for ks in IG_KSPLITS:
                cs.append(_ig(f"mode{mode}-{tile}-nkt7-ksplit{ks}", 129, 224, N, mode, ksplit=ks, beta=1))
            cs.append(_ig(f"mode{mode}-{tile}-nkt7-partial-ksplit3", 127, 196, N, mode, ksplit=3))           # split-K with a partial last tile
            cs.append(_ig(f"mode{mode}-{tile}-nkt17-ksplit2", 129, 544, N, mode, ksplit=2))                  # 9 tiles per split: a fold inside a split
            cs.append(_ig(f"mode{mode}-{tile}-batch3-sharedW", 129, 36, N, mode, nbatch=3, shared_w=True))
            cs.append(_ig(f"mode{mode}-{tile}-batch3-ownW", 129, 36, N, mode, nbatch=3, shared_w=False, beta=1, relu=True))
            cs.append(_ig(f"mode{mode}-{tile}-batch3-ksplit3-ignored", 129, 224, N, mode, nbatch=3, shared_w=False, ksplit=3))
        for N in IG_NOUT[mode]:
            cs.append(_ig(f"mode{mode}-Nout{N}", 129, 36, N, mode))
    return cs


def _igc(name, N, H, W, Kc, Nout, k, stride, pad, dil, mode, **kw):
    """a conv case by the CONV's input size H x W: mode 0 computes the conv, mode 1 its input gradient (X of the launch = dY of the conv, the launch's
    Ho x Wo = H x W)"""
    h, w = conv_out_size(H, k, stride, pad, dil), conv_out_size(W, k, stride, pad, dil)
    a = dict(alpha=-0.5, bias=True, beta=0, relu=False, nbatch=1, shared_w=True, ksplit=0)
    a.update(kw)
    if mode == 0:
        return _IG(name, N, H, W, Kc, h, w, Nout, k, k, stride, pad, dil, 0, **a)
    return _IG(name, N, h, w, Kc, H, W, Nout, k, k, stride, pad, dil, 1, **a)


def igemm_conv_cases():
    cs = []
    for mode in (0, 1):
        m = f"mode{mode}"
        cs += [_igc(f"{m}-1x1-image-3x3-pad1", 2, 1, 1, 32, 64, 3, 1, 1, 1, mode),
               _igc(f"{m}-2x5-map-5x5-pad2", 1, 2, 5, 32, 68, 5, 1, 2, 1, mode, beta=1),
               _igc(f"{m}-stride2-dil2-odd-9x13", 1, 9, 13, 32, 64, 3, 2, 2, 2, mode),
               _igc(f"{m}-stride2-dil2-even-8x12", 1, 8, 12, 96, 132, 3, 2, 2, 2, mode, relu=True),
               _igc(f"{m}-3-images-9x13-Kc32", 3, 9, 13, 32, 132, 3, 1, 1, 1, mode),
               _igc(f"{m}-3-images-9x13-Kc96", 3, 9, 13, 96, 60, 3, 1, 1, 1, mode),
               _igc(f"{m}-3x3-ksplit3-ignored", 1, 9, 13, 32, 64, 3, 1, 1, 1, mode, ksplit=3)]
    for Nout in (64, 96):
        cs += [_igc(f"smallc-7x7-stride2-pad3-Nout{Nout}", 1, 17, 21, 4, Nout, 7, 2, 3, 1, 0),           # 49 taps: 7 tap tiles, one tap in the last
               _igc(f"smallc-3x3-pad1-Nout{Nout}", 2, 9, 13, 4, Nout, 3, 1, 1, 1, 0, relu=True)]          # 9 taps: one tap in the second tile
    return cs


class IgemmProblem:
    """operands of an igemm case in guarded buffers, and its fp64 restatement"""
    def __init__(self, c):
        self.c = c
        s = seed_of("igemm" + c.name)
        taps = c.KH * c.KW
        self.M = c.N_img * c.Ho * c.Wo
        xrows = c.N_img * c.Hi * c.Wi
        self.ldx, self.ldc = c.Kc + 4, c.Nout + 3
        wrows, wcols = (c.Nout, taps * c.Kc) if c.mode == 0 else (c.Kc * taps, c.Nout)
        self.ldw = wcols + (8 if c.mode == 0 else 4)
        nbw = 1 if c.shared_w else c.nbatch
        x = randn(c.nbatch, xrows, c.Kc, seed=s)
        w = randn(nbw, wrows, wcols, seed=s + 1)
        self.bias = randn(c.Nout, seed=s + 2) if c.bias else None
        out0 = randn(c.nbatch, self.M, c.Nout, seed=s + 3) if c.beta else None
        self.sX, self.sC = xrows * self.ldx + 8, self.M * self.ldc + 5
        self.sW = 0 if c.shared_w else wrows * self.ldw + 12
        self.X = Guarded(c.nbatch, xrows, c.Kc, self.ldx, self.sX, fill="nan", data=x)
        self.W = Guarded(nbw, wrows, wcols, self.ldw, self.sW or None, fill="nan", data=w)
        self.out = Guarded(c.nbatch, self.M, c.Nout, self.ldc, self.sC, fill="sentinel", data=out0)
        self.ws = Guarded(1, 1, c.ksplit * self.M * c.Nout, c.ksplit * self.M * c.Nout, fill="sentinel") if c.ksplit > 1 else None
        # the contraction
        if taps == 1 and c.Hi == 1 and c.Wi == 1:
            self.A = x.double()
        else:
            assert c.nbatch == 1
            gather = im2col if c.mode == 0 else im2col_dgrad
            self.A = gather(x[0].double().reshape(c.N_img, c.Hi, c.Wi, c.Kc), c.KH, c.KW, c.stride, c.pad, c.dil, c.Ho, c.Wo)[None]
        if c.mode == 0:
            self.B = w.double().transpose(1, 2)                                                           # [n][(tap, c)] -> [(tap, c)][n]
        else:
            self.B = w.double().reshape(nbw, c.Kc, taps, c.Nout).transpose(1, 2).reshape(nbw, taps * c.Kc, c.Nout)      # [(c, tap)][n] -> [(tap, c)][n]
        self.out0 = out0
        self.chain = chain_igemm(c.Kc, taps, c.ksplit, c.nbatch, c.mode)
        self.K = taps * c.Kc

    def reference(self, drop=None):
        return reference(self.A, self.B, self.c.alpha, self.bias, self.out0, self.c.relu, drop)


# ====================================================================================================================
# skinny cases
# ====================================================================================================================
_SK = namedtuple("SkinnyCase", "name M N K layout alpha bias relu ldc_pad c_offset")

SK_M = (1, 3, 15, 16, 17, 33, 48, 64)
SK_K = (16, 32, 48, 64, 80, 128, 1040)
SK_N = {0: (16, 32, 528, 4112), 1: (64, 128, 576)}


def _sk(name, M, N, K, layout, *, alpha=0.5, bias=True, relu=False, ldc_pad=4, c_offset=0):
    return _SK(name, M, N, K, layout, alpha, bias, relu, ldc_pad, c_offset)


def skinny_cases():
    cs = []
    for layout in (0, 1):
        n0 = SK_N[layout][0]
        for M in SK_M:
            cs.append(_sk(f"layout{layout}-M{M}", M, n0 * 2, 80, layout))                 # one slice of 80 k (five blocks: wave 0 has two)
            cs.append(_sk(f"layout{layout}-M{M}-slices", M, n0, 128, layout))             # two slices of 64 k
        for K in SK_K:
            cs.append(_sk(f"layout{layout}-K{K}", 17, n0, K, layout))                     # K = 1040: nine slices, the last of 16 k
        for N in SK_N[layout]:
            cs.append(_sk(f"layout{layout}-N{N}", 17, N, 128, layout))
        cs.append(_sk(f"layout{layout}-N{SK_N[layout][-2]}-K1040", 33, SK_N[layout][-2], 1040, layout))
        for bias in (False, True):
            for relu in (False, True):
                for alpha in (1.0, 0.5):
                    e = f"bias{int(bias)}relu{int(relu)}alpha{alpha}"
                    cs.append(_sk(f"layout{layout}-{e}-one-slice", 33, n0 * 2, 48, layout, alpha=alpha, bias=bias, relu=relu))
                    cs.append(_sk(f"layout{layout}-{e}-slices", 33, n0 * 2, 1040, layout, alpha=alpha, bias=bias, relu=relu))
    for M, N, K in ((17, 32, 80), (3, 4112, 128), (64, 16, 48)):                          # nsplit == 1: element-wise stores to an unaligned C
        cs.append(_sk(f"layout0-M{M}-N{N}-K{K}-C-off-by-one-float-ldc-N+1", M, N, K, 0, ldc_pad=1, c_offset=1))
    return cs


class SkinnyProblem:
    def __init__(self, c):
        self.c = c
        s = seed_of("skinny" + c.name)
        self.lda, self.ldc = c.K + 4, c.N + c.ldc_pad
        brows, bcols = (c.N, c.K) if c.layout == 0 else (c.K, c.N)
        self.ldb = bcols + 4
        a, b = randn(1, c.M, c.K, seed=s), randn(1, brows, bcols, seed=s + 1)
        self.bias = randn(c.N, seed=s + 2) if c.bias else None
        self.A_buf = Guarded(1, c.M, c.K, self.lda, fill="nan", data=a)
        self.B_buf = Guarded(1, brows, bcols, self.ldb, fill="nan", data=b)
        self.out = Guarded(1, c.M, c.N, self.ldc, fill="sentinel", offset=c.c_offset)
        self.A = a.double()
        self.B = b.double().transpose(1, 2) if c.layout == 0 else b.double()
        self.nsplit = skinny_plan(c.N, c.K, c.layout)[1]
        self.chain = chain_skinny(c.N, c.K, c.layout)
        self.K = c.K

    def reference(self, drop=None):
        return reference(self.A, self.B, self.c.alpha, self.bias, None, self.c.relu, drop)


# calls outside the domain include/scanpaths_amd.h states: (name, M, N, K, lda pad, ldb pad, ldc pad, layout, byte offsets of A, B, C, bias,
# workspace, expected code).  Pads are added to the widths (K; K or N; N).  rc -1 = SP_EINVAL.  `shape` rows are those sp_gemm_skinny_applies can
# see (it gets no pointers, and of ldc only what layout 1 asks): there it must return 0; in the pointer rows it returns 1.
_RF = namedtuple("Refusal", "name M N K lda_pad ldb_pad ldc_pad layout offA offB offC offBias offWs rc applies")


def _rf(name, M, N, K, layout, *, lda_pad=4, ldb_pad=4, ldc_pad=4, offA=0, offB=0, offC=0, offBias=0, offWs=0, rc=-1, applies=0):
    return _RF(name, M, N, K, lda_pad, ldb_pad, ldc_pad, layout, offA, offB, offC, offBias, offWs, rc, applies)


def skinny_refusals():
    return [
        _rf("M0", 0, 32, 64, 0), _rf("M65", 65, 32, 64, 0), _rf("M65-layout1", 65, 64, 64, 1),
        _rf("K8", 17, 32, 8, 0), _rf("K24", 17, 32, 24, 0), _rf("K24-layout1", 17, 64, 24, 1),
        _rf("N8-layout0", 17, 8, 64, 0), _rf("N24-layout0", 17, 24, 64, 0), _rf("N96-layout1", 17, 96, 64, 1),
        _rf("lda%4", 17, 32, 64, 0, lda_pad=2), _rf("lda%4-layout1", 17, 64, 64, 1, lda_pad=2),
        _rf("layout2", 17, 64, 64, 2),
        _rf("A+4B", 17, 32, 64, 0, offA=4, applies=1), _rf("B+4B", 17, 32, 64, 0, offB=4, applies=1),
        _rf("A+4B-layout1", 17, 64, 64, 1, offA=4, applies=1), _rf("B+4B-layout1", 17, 64, 64, 1, offB=4, applies=1),
        _rf("workspace+4B", 17, 32, 128, 0, offWs=4, applies=1), _rf("workspace+4B-layout1", 17, 64, 1040, 1, offWs=4, applies=1),
        _rf("C+4B-layout1", 17, 64, 48, 1, offC=4, applies=1), _rf("bias+4B-layout1", 17, 64, 48, 1, offBias=4, applies=1),
        _rf("C+4B-slices", 17, 32, 128, 0, offC=4, applies=1), _rf("bias+4B-slices", 17, 32, 128, 0, offBias=4, applies=1),
        _rf("ldc%4-slices", 17, 32, 128, 0, ldc_pad=2, applies=1),          # layout 0 asks nothing of ldc until slices are used: the entry point refuses
        _rf("ldc%4-layout1", 17, 64, 48, 1, ldc_pad=2),
        # an offset of None passes NULL: SP_ENULL (-2) for a required pointer, and for the workspace once slices are used
        _rf("A-null", 17, 32, 64, 0, offA=None, rc=-2, applies=1), _rf("B-null", 17, 64, 64, 1, offB=None, rc=-2, applies=1),
        _rf("C-null", 17, 32, 64, 0, offC=None, rc=-2, applies=1), _rf("workspace-null-slices", 17, 32, 128, 0, offWs=None, rc=-2, applies=1),
    ]


# ====================================================================================================================
# wgrad cases
# ====================================================================================================================
_WG = namedtuple("WgradCase", "name N_img Hi Wi Ci Ho Wo Co KH KW stride pad dil alpha beta nbatch")

WG_ROWS = (1, 31, 32, 33, 257, 513, 2049)
WG_CO = (4, 124, 128, 132)
WG_CI = (4, 60, 128, 132)


def _wg(name, rows, Co, Ci, *, alpha=-0.5, beta=0, nbatch=1):
    return _WG(name, rows, 1, 1, Ci, 1, 1, Co, 1, 1, 1, 0, 1, alpha, beta, nbatch)


def _wgc(name, N, H, W, Ci, Co, k, stride, pad, dil, *, alpha=-0.5, beta=0):
    return _WG(name, N, H, W, Ci, conv_out_size(H, k, stride, pad, dil), conv_out_size(W, k, stride, pad, dil), Co, k, k, stride, pad, dil, alpha,
               beta, 1)


def wgrad_cases(extra_rows=()):
    cs = []
    for rows in WG_ROWS + tuple(extra_rows):
        cs.append(_wg(f"rows{rows}", rows, 132, 60))
    for Co in WG_CO:
        cs.append(_wg(f"Co{Co}", 33, Co, 132))
        cs.append(_wg(f"Co{Co}-rows2049", 2049, Co, 4))
    for Ci in WG_CI:
        cs.append(_wg(f"Ci{Ci}", 33, 124, Ci))
        cs.append(_wg(f"Ci{Ci}-rows513", 513, 4, Ci))
    for beta in (0, 1):
        for alpha in (1.0, -0.5):
            cs.append(_wg(f"beta{beta}alpha{alpha}-rows257", 257, 132, 60, alpha=alpha, beta=beta))
            cs.append(_wg(f"beta{beta}alpha{alpha}-rows2049", 2049, 132, 60, alpha=alpha, beta=beta))
    cs.append(_wg("batch3", 33, 132, 60, nbatch=3))
    cs.append(_wg("batch3-beta1-rows513", 513, 124, 132, nbatch=3, beta=1))
    cs += [_wgc("conv-3x3-pad1-Ci4", 2, 9, 13, 4, 132, 3, 1, 1, 1),                       # Ntot = 36: a column tile spans nine taps
           _wgc("conv-3x3-stride2-dil2-pad2", 2, 9, 13, 60, 124, 3, 2, 2, 2, beta=1),
           _wgc("conv-3x3-stride2-dil2-pad2-even", 1, 8, 12, 32, 4, 3, 2, 2, 2),
           _wgc("conv-1x1-image-3x3", 3, 1, 1, 60, 128, 3, 1, 1, 1),
           _wgc("conv-7x7-stride2-Ci4", 2, 33, 41, 4, 64, 7, 2, 3, 1),                    # Ntot = 196: two column tiles; 714 pixels
           _wgc("conv-3x3-pad1-slabs", 3, 17, 21, 32, 64, 3, 1, 1, 1, beta=1)]            # 1071 pixels
    return cs


class WgradProblem:
    def __init__(self, c):
        self.c = c
        s = seed_of("wgrad" + c.name)
        taps = c.KH * c.KW
        self.M, self.Ntot = c.N_img * c.Ho * c.Wo, taps * c.Ci
        xrows = c.N_img * c.Hi * c.Wi
        self.ldx, self.ldy, self.ldo = c.Ci + 4, c.Co + 4, self.Ntot + 4
        x, dy = randn(c.nbatch, xrows, c.Ci, seed=s), randn(c.nbatch, self.M, c.Co, seed=s + 1)
        out0 = randn(c.nbatch, c.Co, self.Ntot, seed=s + 2) if c.beta else None
        self.sX, self.sY, self.sO = xrows * self.ldx + 8, self.M * self.ldy + 12, c.Co * self.ldo + 5
        self.X = Guarded(c.nbatch, xrows, c.Ci, self.ldx, self.sX, fill="nan", data=x)
        self.dY = Guarded(c.nbatch, self.M, c.Co, self.ldy, self.sY, fill="nan", data=dy)
        self.out = Guarded(c.nbatch, c.Co, self.Ntot, self.ldo, self.sO, fill="sentinel", data=out0)
        self.A = dy.double().transpose(1, 2)
        if taps == 1 and c.Hi == 1 and c.Wi == 1:
            self.B = x.double()
        else:
            assert c.nbatch == 1
            self.B = im2col(x[0].double().reshape(c.N_img, c.Hi, c.Wi, c.Ci), c.KH, c.KW, c.stride, c.pad, c.dil, c.Ho, c.Wo)[None]
        self.out0 = out0
        self.K = self.M

    def desc(self, hip):
        c = self.c
        return hip.WgradDesc(N_img=c.N_img, Hi=c.Hi, Wi=c.Wi, Ci=c.Ci, ldx=self.ldx, Ho=c.Ho, Wo=c.Wo, Co=c.Co, ldy=self.ldy, KH=c.KH, KW=c.KW,
                             stride=c.stride, pad=c.pad, dil=c.dil, ldo=self.ldo, beta=c.beta, alpha=c.alpha, nbatch=c.nbatch,
                             strideX=self.sX if c.nbatch > 1 else 0, strideY=self.sY if c.nbatch > 1 else 0,
                             strideO=self.sO if c.nbatch > 1 else 0)

    def reference(self, drop=None):
        return reference(self.A, self.B, self.c.alpha, None, self.out0, False, drop)


def empty_split_rows(lib, hip, limit=20000):
    """row counts <= limit of a TN GEMM at which sp_conv_wgrad's plan leaves its last split without a row (rows_per_split is rounded up to 32, so
    (splits - 1) rows_per_split can reach the row count), for every tile count of the case lists (1, 2, 4 tiles)"""
    import ctypes
    found = []
    for Co, Ci in ((128, 128), (132, 128), (132, 132)):
        for rows in range(1, limit + 1):
            d = hip.WgradDesc(N_img=rows, Hi=1, Wi=1, Ci=Ci, ldx=Ci, Ho=1, Wo=1, Co=Co, ldy=Co, KH=1, KW=1, stride=1, pad=0, dil=1, ldo=Ci, beta=0,
                              alpha=1.0, nbatch=1)
            s = lib.sp_conv_wgrad_workspace(ctypes.byref(d)) // (Co * Ci * 4)
            if s > 1 and (s - 1) * cdiv(cdiv(rows, s), 32) * 32 >= rows:
                found.append((Co, Ci, rows, s))
    return found
