"""Plain restatement of the 2xfp16 kernels of csrc/conv_f16x2.hip -- the operand splitters bit for bit, and every GEMM launch as one fp64
contraction -- the reference side of tests/test_f16x2_ref_cpu.py and tests/test_conv_f16x2_gpu.py.  Nothing here touches a GPU.

OPERANDS.  x * s = x1 + x2 with a power-of-two scale s (scale_of), x1 = fp16(x s), x2 = fp16(x s - x1) (split2), stored as
[row][K / 16][plane][16] fp16 followed by a 64-byte zero block (pack).  The five entry points differ only in what a row is and which maximum sets
the scale (split2_f16, split2_f16_wT, split2_f16_rows, split2_f16_wT_rows, split2_f16_cols below).

TWO CONTRACTIONS PER LAUNCH, both in fp64:
    R_planes   what the kernel is asked to compute: the decoded planes with exactly the products the build takes (NPROD = 3: a1 b1 + a1 b2 +
               a2 b1; NPROD = 1: a1 b1), divided by the scales, then the epilogue of the ABI
    R_true     the same contraction on the fp32 operands
The gathers are gemm_ref.im2col / im2col_dgrad; the weight operand is always [Nout][K] with k = (tap, channel).

TWO BARS, both derived, neither tuned on results:
    kernel against R_planes   parity.bar(S, c): c 2^-24 S + 2^-149, with S the contraction over absolute values of the planes (a subnormal plane
                              entry counted at the format's smallest exponent: hw_abs), c the launch's longest chain of dependent roundings in
                              units of 2^-24 (chain_h2, chain_hw, chain_hw2).
                              ASSUMPTION (nobody here has measured what v_mfma_f32_16x16x32_f16 does inside one instruction and the
                              microarchitecture notes only state that the fp32-input MFMAs are exact fmaf chains): fp16 x fp16 products are
                              exact in fp32, and every product of the 32 an instruction adds into its accumulator costs ONE TRUNCATION, 2^-23 =
                              two units (PROD_UNITS).  A K-tile is three such instructions (NPROD = 3) into the same accumulator.
    R_planes against R_true   rep_bound: the representation error of split2, derived there.

LATTICE DATA.  Scaled values h + l with h in {-4096, 0, 4096}, l in {-1, 0, 1} (0 where h = 0) and one 8192 per scale group, the fp32 inputs these
divided by a power of two: then x1 = h and x2 = l exactly, every product and partial sum is a multiple of 4096, and as long as
S / 4096 <= 2^24 every fp32 accumulation order gives the bits of the fp64 sum (the `rich` variant: h = 1024 p, p in 4..7, granularity 1024).
With a power-of-two alpha and bias / out0 on the same lattice the epilogue is exact too: the kernel must equal R_planes BIT FOR BIT."""
from collections import namedtuple

import numpy as np
import torch

from gemm_ref import conv_out_size, im2col, im2col_dgrad
from parity import U, cdiv, seed_of

F32, F16 = np.float32, np.float16
PROD_UNITS = 2          # one truncation (2^-23) per product, in units of 2^-24: the assumption of the module docstring
HCHUNK_KT = 8           # K-tiles between two folds of `acc` into `tot` (h2_kernel and hw_kernel)
F16_NAN = 0x7E00


# ====================================================================================================================
# (a) the splitters, bit for bit
# ====================================================================================================================
def scale_of(amax):
    """common.h scale_of: the power of two s with amax s in [8192, 16384); 1 for a maximum that is zero, infinite or NaN; e clamped to +-126"""
    a = F32(amax)
    if not (a > 0) or not np.isfinite(a):
        return F32(1.0)
    e = 14 - int(np.frexp(a)[1])
    return np.ldexp(F32(1.0), max(-126, min(126, e)))


def scales_of(amax):
    return np.array([scale_of(a) for a in np.asarray(amax).reshape(-1)], dtype=F32).reshape(np.shape(amax))


def split2(v, s):
    """common.h split2, element-wise: (x1, x2) fp16"""
    with np.errstate(over="ignore", invalid="ignore"):
        xs = (np.asarray(v, dtype=F32) * np.asarray(s, dtype=F32)).astype(F32)
        x1 = xs.astype(F16)
        x2 = (xs - x1.astype(F32)).astype(F32).astype(F16)
    return x1, x2


def pack(x1, x2, ld=None):
    """[rows][K] planes -> uint16 [rows][ld / 16][2][16] + 32 zero halves; columns K .. ld - 1 (wider rows) hold fp16 NaNs"""
    rows, K = x1.shape
    ld = K if ld is None else ld
    assert ld % 16 == 0 and K <= ld
    buf = np.full((2, rows, ld), F16_NAN, dtype=np.uint16)
    buf[0, :, :K], buf[1, :, :K] = x1.view(np.uint16), x2.view(np.uint16)
    out = buf.reshape(2, rows, ld // 16, 16).transpose(1, 2, 0, 3)
    return np.concatenate([out.reshape(-1), np.zeros(32, np.uint16)])


def unpack(planes, rows, K, ld=None):
    """the inverse of pack: (x1, x2) fp64 [rows][K]"""
    ld = K if ld is None else ld
    p = np.asarray(planes[:2 * rows * ld]).view(F16).reshape(rows, ld // 16, 2, 16)
    return (p[:, :, 0].reshape(rows, ld)[:, :K].astype(np.float64), p[:, :, 1].reshape(rows, ld)[:, :K].astype(np.float64))


def _amax(x):
    x = np.abs(np.asarray(x, dtype=F32))
    return F32(np.fmax.reduce(x.reshape(-1))) if x.size else F32(0)          # fmaxf: a NaN operand is ignored


def split2_f16(x, bound=None):
    """sp_split2_f16: x fp32 [n] (any shape, n % 16 == 0) -> (planes, scale); bound: the value scale_amax[1] holds under have_amax = 1"""
    x = np.asarray(x, dtype=F32).reshape(1, -1)
    s = scale_of(_amax(x) if bound is None else bound)
    return pack(*split2(x, s)), s


def split2_f16_wT(w):
    """sp_split2_f16_wT: w [Co][taps][Ci] -> rows ci, k = (tap, co), one scale"""
    w = np.asarray(w, dtype=F32)
    Co, taps, Ci = w.shape
    s = scale_of(_amax(w))
    return pack(*split2(w.transpose(2, 1, 0).reshape(Ci, taps * Co), s)), s


def split2_f16_rows(w, Kc=0, absorb=None):
    """sp_split2_f16_rows: w [rows][K] -> planes of w[r][tap][c] / absorb[c], one scale per row"""
    w = np.asarray(w, dtype=F32)
    if absorb is not None:
        w = (w / np.tile(np.asarray(absorb, dtype=F32), w.shape[1] // Kc)[None]).astype(F32)
    s = scales_of(np.array([_amax(r) for r in w]))
    return pack(*split2(w, s[:, None])), s


def split2_f16_wT_rows(w, absorb=None):
    """sp_split2_f16_wT_rows: w [nbatch][Co][taps][Ci] -> rows (item, ci), k = (tap, co), value w * (1 / absorb[co]), one scale per row"""
    w = np.asarray(w, dtype=F32)
    nb, Co, taps, Ci = w.shape
    if absorb is not None:
        w = (w * (F32(1.0) / np.asarray(absorb, dtype=F32))[None, :, None, None]).astype(F32)
    v = w.transpose(0, 3, 2, 1).reshape(nb * Ci, taps * Co)
    s = scales_of(np.array([_amax(r) for r in v]))
    return pack(*split2(v, s[:, None])), s


def split2_f16_cols(x):
    """sp_split2_f16_cols: x [rows][C] -> planes of x * s_c; an all-zero channel gets 2^100"""
    x = np.asarray(x, dtype=F32)
    m = np.fmax.reduce(np.abs(x), axis=0)
    s = np.array([scale_of(a) if a > 0 else F32(2.0 ** 100) for a in m], dtype=F32)
    return pack(*split2(x, s[None])), s


def colamax_blocks(rows, C):
    """colamax_blocks of the library: sp_split2_f16_cols_workspace = blocks * C * 4 bytes"""
    rpb = 256 // min(C // 4, 256)
    return max(1, min(cdiv(rows, rpb * 4), 512))


# ====================================================================================================================
# (c) chains of dependent roundings, in units of 2^-24
# ====================================================================================================================
def hw_abs(x):
    """the magnitude of a plane entry AS THE INSTRUCTION ALIGNS IT: |x|, but 2^-14 for a non-zero fp16 subnormal.  A subnormal operand is not
    normalised: it carries the format's smallest exponent, 2^-14, with leading zeros in its significand, and the truncation of a product (2^-23 of
    the largest addend, the assumption of the module docstring) is taken from that exponent, not from the value.  Measured on the first run of
    tests/test_conv_f16x2_gpu.py (profiles/conv_f16x2_parity.md): a1 = 2^-24 (subnormal), b1 = 257.5, b2 = -509 2^-12 gave a1 b1 + a1 b2 with
    a1 b2 cut to a multiple of 2^-30 = 24 bits below the FORMAT exponent 2^-6 of a1 b1, whose value is 2^-16.  S, the contraction over absolute
    values the bar scales with, is taken over these magnitudes; for entries that are normal fp16 numbers nothing changes."""
    a = x.abs()
    return torch.where((a > 0) & (a < 2.0 ** -14), torch.full_like(a, 2.0 ** -14), a)


def _chain(n):
    """(1 + u)^n - 1 <= n u (1 + 2 n u) while n u <= 1/2; plus one unit for the fp64 reference's own error"""
    assert n * U <= 0.5
    return int(np.ceil(n * (1 + 2 * n * U))) + 1


def chain_h2(Kc, taps, nprod=3):
    """h2_kernel: a K-tile is nprod v_mfma_f32_16x16x32_f16 of 32 k into ONE accumulator: 32 nprod products of PROD_UNITS each, at most
    HCHUNK_KT = 8 tiles before `acc` is folded into `tot` (fold: ((kt + 1) & 7) == 0) and restarted; one add per fold, nkt // 8 folds and the
    epilogue's tot + acc; the epilogue multiplies by 1 / sx, 1 / sw and alpha and adds bias and out: 5 (the scale factors are powers of two and
    cost nothing; they are counted all the same)."""
    nkt = taps * Kc // 32
    return _chain(PROD_UNITS * 32 * nprod * min(HCHUNK_KT, nkt) + (nkt // HCHUNK_KT + 1) + 5)


def hw_rows_per_split(M, splits):
    return cdiv(cdiv(M, splits), 32) * 32


def chain_hw(M, splits, nprod=3):
    """hw_kernel + hw_reduce(4)_kernel: a K-tile is 32 pixels, nprod instructions into one accumulator, chunks and folds as in h2_kernel
    (fold: (kt & 7) == 7).  Direct (one split, or a batch item): 1 / sx, 1 / sy, alpha, beta * out: 4.  Through slabs: the reducer adds the
    `splits` slabs onto 0.f, multiplies by 1 / sx and 1 / sy, adds onto acc = 0.f, multiplies by alpha, adds out: splits + 5."""
    nkt = cdiv(min(M, hw_rows_per_split(M, splits)), 32)
    return _chain(PROD_UNITS * 32 * nprod * min(HCHUNK_KT, nkt) + (nkt // HCHUNK_KT + 1) + (4 if splits <= 1 else splits + 5))


def chain_hw2(M, splits, nseg):
    """hw2_kernel + reducer: SINGLE-level accumulation over the split's pixels (3 instructions per 32-pixel K-tile, no folds); the reducer adds
    `splits` slabs, scales twice, adds the nseg applications one after another, multiplies by alpha, adds out."""
    nkt = hw_rows_per_split(M, splits) // 32
    return _chain(PROD_UNITS * 32 * 3 * nkt + splits + 2 + nseg + 2)


# ====================================================================================================================
# (e) the plans of the product build (tuning values at their defaults)
# ====================================================================================================================
def hw_splits(M, Co, Ntot):
    """hw_splits of conv_f16x2.hip: the cost rule rounds x (K-tiles of a split + 12 + splits / 2), rounds = ceil(tiles splits / 256)"""
    tiles = cdiv(Co, 256) * cdiv(Ntot, 128)
    best, best_cost = 1, 1e30
    for sp in range(1, min(128, max(1, M // 1024)) + 1):
        cost = float(cdiv(tiles * sp, 256)) * (float(cdiv(cdiv(M, sp), 32)) + 12.0 + 0.5 * sp)
        if cost < best_cost * 0.999:
            best, best_cost = sp, cost
    return best


def hw2_applies(c, nseg, ldo):
    M = c.N_img * c.Ho * c.Wo
    return (1 <= nseg <= 16 and c.nbatch == 1 and c.stride == 1 and c.Wo % 32 == 0 and c.Co % 256 == 0 and c.Ci % 16 == 0
            and (c.KH * c.KW * c.Ci) % 256 == 0 and ldo % 4 == 0 and ldo >= c.KH * c.KW * c.Ci and M >= 2048)


def hw2_splits(M, Co, Ntot, nseg):
    """hw2_splits: chains of at most 20480 pixels, >= 64 K-tiles per workgroup, between them rounds x (K-tiles + 20 + splits / 2)"""
    tiles = (Co // 256) * (Ntot // 256)
    smin = cdiv(M, 20480)
    best, best_cost = smin, 1e30
    for sp in range(smin, max(smin, M // 2048) + 1):
        cost = float(cdiv(tiles * nseg * sp, 256)) * (float(cdiv(cdiv(M, sp), 32)) + 20.0 + 0.5 * sp)
        if cost < best_cost * 0.999:
            best, best_cost = sp, cost
    return max(1, best)


def halo_applies(c):
    return (c.KH == 3 and c.KW == 3 and c.stride == 1 and c.dil == 1 and c.pad == 1 and c.Wo == 64 and c.Wi == 64 and c.Hi == c.Ho
            and (c.Ho * c.Wo) % 256 == 0 and c.Kc % 32 == 0)


def cbm_ok(c):
    return 1 < c.KH * c.KW <= 32 and (c.mode == 0 or c.stride == 1)


def row_nimg(c, has_row_last):
    """the live-first tile order of the row-sparse data gradient: samples, or 0 for the plain order"""
    return c.N_img if (has_row_last and c.mode == 1 and c.nbatch == 1 and c.N_img <= 64 and (c.Ho * c.Wo) % 256 == 0) else 0


def h2_build(c):
    """the h2_kernel build conv_igemm_f16 selects: <MODE, NPROD, CBM, HALO> as a name"""
    stats = getattr(c, "stats", False)
    if c.nprod == 1:
        order = "tap-major"
    elif cbm_ok(c) and halo_applies(c) and not stats:
        order = "halo"
    else:
        order = "cbm" if cbm_ok(c) else "tap-major"
    return f"h2<mode{c.mode},nprod{c.nprod},{order}>" + ("+stats" if stats else "")


def hw_reducer(Ntot, ldo, Co, Ci):
    """launch_hw_reduce's choice (bases 16-byte aligned, as every case here passes them)"""
    return "hw_reduce4" if Ntot % 4 == 0 and ldo % 4 == 0 and (Co * ldo) % 4 == 0 and Ci % 4 == 0 else "hw_reduce"


# ====================================================================================================================
# data
# ====================================================================================================================
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def gauss(shape, seed):
    return _rng(seed).standard_normal(shape).astype(F32)


def heavy(shape, seed):
    """heavy-tailed gradients as in test_split_gemms_are_as_accurate_as_cpu_fp32: randn * rand^4"""
    g = _rng(seed)
    return (g.standard_normal(shape) * g.random(shape) ** 4).astype(F32)


def lattice(shape, group_axes, seed, rich=False, keep=None, qmax=4):
    """(x fp32, h, l): x = (h + l) / 2^q, one 8192 per scale group, q in 0 .. qmax - 1 per group.  group_axes: the axes that index the scale
    groups (() = one group).  keep: the share of non-zero h where the default (2/3; rich: 1/2) would exceed the exactness condition -- the sum
    over several applications in sp_conv_wgrad_f16x2_multi."""
    g = _rng(seed)
    if rich:
        h = 1024 * g.integers(4, 8, shape) * g.choice([-1, 1], shape) * (g.random(shape) < 0.5)
    elif keep is not None:
        h = 4096 * g.choice([-1, 1], shape) * (g.random(shape) < keep)
    else:
        h = 4096 * g.integers(-1, 2, shape)
    l = g.integers(-1, 2, shape) * (h != 0)
    gshape = tuple(shape[a] if a in group_axes else 1 for a in range(len(shape)))
    other = [a for a in range(len(shape)) if a not in group_axes]
    # the pin: one position per group
    hm = np.moveaxis(h, other, range(len(shape) - len(other), len(shape))).reshape(int(np.prod(gshape)), -1)
    lm = np.moveaxis(l, other, range(len(shape) - len(other), len(shape))).reshape(hm.shape)
    pos = g.integers(0, hm.shape[1], hm.shape[0])
    hm[np.arange(hm.shape[0]), pos], lm[np.arange(hm.shape[0]), pos] = 8192, 0
    gs = tuple(shape[a] for a in group_axes) + tuple(shape[a] for a in other)
    back = lambda m: np.moveaxis(m.reshape(gs), range(len(group_axes), len(shape)), other) if group_axes else m.reshape(shape)
    h, l = back(hm), back(lm)
    q = g.integers(0, qmax, gshape)
    x = ((h + l) / 2.0 ** q).astype(F32)
    return x, h.astype(np.float64), l.astype(np.float64)


def make(kind, shape, group_axes, seed, rich=False, **lattice_kw):
    if kind == "lattice":
        return lattice(shape, group_axes, seed, rich, **lattice_kw)[0]
    return gauss(shape, seed) if kind == "gauss" else heavy(shape, seed)


# ====================================================================================================================
# (c) the representation bound
# ====================================================================================================================
def rep_bound(absA, absB, nprod):
    """|sum_k as bs - (the products the build takes)| element-wise, for scaled operands as = a s, bs = b s ([.., M, K] x [.., K, N], fp64 absolute
    values).  split2: as = a1 + a2 + ea with |as - a1| <= h |as| + t and |ea| <= h^2 |as| + t, h = 2^-11 (fp16 round to nearest), t = 2^-25 (half
    the fp16 subnormal spacing), so |a2| <= d(as) = h (1 + h) |as| + 2 t.
      NPROD = 3:  as bs - (a1 b1 + a1 b2 + a2 b1) = a2 b2 + ea bs + (as - ea) eb
                  <= d(as) d(bs) + (h^2 |as| + t) |bs| + |as| (h^2 |bs| + t)          (residual 2 x 2^-22 |as bs|, the dropped a2 b2 another 2^-22)
      NPROD = 1:  as bs - a1 b1 = (as - a1) bs + a1 (bs - b1) <= (h |as| + t) |bs| + ((1 + h) |as| + t) (h |bs| + t)      (the 2^-11 term, twice)"""
    h, t = 2.0 ** -11, 2.0 ** -25
    AB = torch.matmul(absA, absB)
    ra, cb, K = absA.sum(-1, keepdim=True), absB.sum(-2, keepdim=True), absA.shape[-1]
    if nprod == 3:
        d1, d0 = h * (1 + h), 2 * t
        return (d1 * d1 + 2 * h * h) * AB + (d1 * d0 + t) * (ra + cb) + K * d0 * d0
    return (h + (1 + h) * h) * AB + t * (1 + h) * cb + t * (1 + h) * ra + K * t * t


# ====================================================================================================================
# igemm (h2_kernel) cases
# ====================================================================================================================
_H2 = namedtuple("H2Case", "name N_img Hi Wi Kc Ho Wo Nout KH KW stride pad dil mode alpha bias beta relu nbatch sw_rows ldx_pad ldc_pad "
                           "nprod stats rich")
_H2_DEF = dict(alpha=-0.5, bias=True, beta=0, relu=False, nbatch=1, sw_rows=False, ldx_pad=16, ldc_pad=3, nprod=3, stats=False, rich=False)


def _hg(name, M, Kc, Nout, mode, **kw):
    return _H2(name, M, 1, 1, Kc, 1, 1, Nout, 1, 1, 1, 0, 1, mode, **{**_H2_DEF, **kw})


def _hc(name, N, H, W, Kc, Nout, k, stride, pad, dil, mode, **kw):
    """a conv case by the CONV's input size: mode 0 computes the conv, mode 1 its input gradient (the launch's Ho x Wo = H x W)"""
    h, w = conv_out_size(H, k, stride, pad, dil), conv_out_size(W, k, stride, pad, dil)
    a = {**_H2_DEF, **kw}
    if mode == 0:
        return _H2(name, N, H, W, Kc, h, w, Nout, k, k, stride, pad, dil, 0, **a)
    return _H2(name, N, h, w, Kc, H, W, Nout, k, k, stride, pad, dil, 1, **a)


H2_M = (1, 255, 256, 257, 513)
H2_NOUT = (1, 127, 128, 129, 260)
H2_KC = (32, 64, 256, 288, 544)          # 1, 2, 8, 9, 17 K-tiles: a ring prologue shorter than the ring, folds at 8 and 16, a remainder


def h2_gemm_cases():
    cs = []
    for mode in (0, 1):
        m = f"mode{mode}"
        for M in H2_M:
            cs.append(_hg(f"{m}-M{M}", M, 64, 129, mode))
        for N in H2_NOUT:
            cs.append(_hg(f"{m}-Nout{N}", 257, 32, N, mode, ldc_pad=4 if N % 2 == 0 else 3))
        for Kc in H2_KC:
            cs.append(_hg(f"{m}-Kc{Kc}", 257, Kc, 129, mode, sw_rows=Kc in (64, 288), rich=Kc <= 256))
        for bias in (False, True):
            for beta in (0, 1):
                for relu in (False, True):
                    e = f"bias{int(bias)}beta{beta}relu{int(relu)}"
                    cs.append(_hg(f"{m}-{e}-scalar-stores", 257, 288, 129, mode, bias=bias, beta=beta, relu=relu))               # Nout % 4 != 0
                    cs.append(_hg(f"{m}-{e}-wide-stores", 513, 96, 260, mode, bias=bias, beta=beta, relu=relu, ldc_pad=4, sw_rows=relu))
        cs.append(_hg(f"{m}-dense-ldx-ldc", 257, 64, 128, mode, ldx_pad=0, ldc_pad=0))
        cs.append(_hg(f"{m}-supertile-4x8", 1024, 32, 1024, mode, ldc_pad=0, bias=False))
        cs.append(_hg(f"{m}-n-fastest", 1024, 32, 896, mode, ldc_pad=4))
    return cs


def h2_conv_cases():
    cs = []
    for mode in (0, 1):
        m = f"mode{mode}"
        cs += [_hc(f"{m}-1x1-image-3x3", 2, 1, 1, 32, 64, 3, 1, 1, 1, mode),
               _hc(f"{m}-2x5-map-5x5", 1, 2, 5, 32, 68, 5, 1, 2, 1, mode, beta=1, ldc_pad=4),
               _hc(f"{m}-3-images-9x13-Kc32", 3, 9, 13, 32, 132, 3, 1, 1, 1, mode, sw_rows=True),
               _hc(f"{m}-3-images-9x13-Kc96", 3, 9, 13, 96, 60, 3, 1, 1, 1, mode, ldc_pad=4, relu=True),
               _hc(f"{m}-dil2-9x13", 2, 9, 13, 32, 64, 3, 1, 2, 2, mode),
               _hc(f"{m}-dil4-9x13", 2, 9, 13, 32, 64, 3, 1, 4, 4, mode, ldx_pad=0),
               _hc(f"{m}-stride2-dil2-9x13", 1, 9, 13, 32, 64, 3, 2, 2, 2, mode),                  # mode 1: tap-major by exclusion
               _hc(f"{m}-stride2-dil2-8x12", 1, 8, 12, 96, 132, 3, 2, 2, 2, mode, relu=True),
               _hc(f"{m}-tall-supertile", 2, 32, 32, 32, 512, 3, 1, 1, 1, mode, ldc_pad=0, bias=False),     # M = 2048, Nout = 512
               _hc(f"{m}-beside-tall-supertile", 7, 16, 16, 32, 512, 3, 1, 1, 1, mode, ldc_pad=4)]         # M = 1792
    cs.append(_hc("mode0-7x7-stride2-49-taps", 1, 9, 13, 32, 64, 7, 2, 3, 1, 0))                            # tap-major: 49 taps > 32
    for mode in (0, 1):
        m = f"mode{mode}-halo"
        cs += [_hc(f"{m}-Ho4", 1, 4, 64, 32, 64, 3, 1, 1, 1, mode),                                        # both halo rows outside the image
               _hc(f"{m}-Ho8-seam", 1, 8, 64, 96, 160, 3, 1, 1, 1, mode, ldc_pad=4, sw_rows=True),
               _hc(f"{m}-Ho12-3-images", 3, 12, 64, 32, 160, 3, 1, 1, 1, mode, beta=1, ldx_pad=0),
               _hc(f"{m}-not-Ho6", 2, 6, 64, 32, 64, 3, 1, 1, 1, mode),                                    # tiles cross images
               _hc(f"{m}-not-Wo32", 1, 8, 32, 32, 64, 3, 1, 1, 1, mode),
               _hc(f"{m}-not-pad2-dil2", 1, 4, 64, 32, 64, 3, 1, 2, 2, mode)]
    return cs


def h2_stats_cases():
    cs = []
    for k, pad in ((3, 1), (1, 0)):
        for (N, H, W), Nout in (((1, 15, 20), 96), ((1, 16, 32), 160), ((1, 15, 20), 160), ((2, 16, 16), 96)):      # M = 300 (ragged), 512
            cs.append(_hc(f"stats-{k}x{k}-M{N * H * W}-Nout{Nout}", N, H, W, 32, Nout, k, 1, pad, 1, 0, bias=False, stats=True,
                          ldc_pad=4 if Nout == 160 else 3, alpha=1.0))
    return cs


def h2_x1_cases():
    """the one-product entry: six cases from the lists above"""
    return [_hg("x1-mode0-M257-Kc288", 257, 288, 129, 0, nprod=1), _hg("x1-mode1-M513-wide", 513, 96, 260, 1, nprod=1, ldc_pad=4, beta=1),
            _hg("x1-mode0-Kc544-rows", 257, 544, 129, 0, nprod=1, sw_rows=True),
            _hc("x1-mode0-3-images-9x13", 3, 9, 13, 32, 132, 3, 1, 1, 1, 0, nprod=1),                      # CBM excluded: tap-major
            _hc("x1-mode1-3-images-9x13", 3, 9, 13, 96, 60, 3, 1, 1, 1, 1, nprod=1, relu=True),
            _hc("x1-mode0-halo-shape", 1, 8, 64, 32, 64, 3, 1, 1, 1, 0, nprod=1)]


def h2_batched_cases():
    """mode 0, nbatch 3, one weight set per item, 256 rows per item; ldc % 4 != 0 and Nout % 4 != 0 reach the scalar tail of the zero-tile writer"""
    return [_hg(f"batch3-Nout{N}-ldc{ldc}-beta{beta}-rows{int(rows)}", 256, 64, N, 0, nbatch=3, ldc_pad=ldc - N, beta=beta, sw_rows=rows)
            for (N, ldc, rows) in ((128, 132, False), (128, 131, True), (130, 132, False)) for beta in (0, 1)]


class H2Problem:
    """operands of an igemm case as packed planes, and its two fp64 restatements.  kind: gauss / heavy / lattice"""
    def __init__(self, c, kind="gauss"):
        self.c, self.kind = c, kind
        s = seed_of("h2" + kind + c.name)
        taps = c.KH * c.KW
        self.K, self.M = taps * c.Kc, c.N_img * c.Ho * c.Wo
        self.xrows = c.N_img * c.Hi * c.Wi
        nb = c.nbatch
        self.nbw = nbw = nb                                                                            # batched: one weight set per item
        self.ldx, self.ldc = c.Kc + c.ldx_pad, c.Nout + c.ldc_pad
        x = make(kind, (nb, self.xrows, c.Kc), (), s, c.rich)
        w = make(kind, (nbw, c.Nout, self.K), (0, 1) if c.sw_rows else (), s + 1, c.rich)
        self.x, self.w = x, w
        self.sx = scale_of(_amax(x))
        self.sw = scales_of(np.array([_amax(r) for r in w.reshape(nbw * c.Nout, -1)])) if c.sw_rows else np.full(1, scale_of(_amax(w)), F32)
        swn = self.sw.reshape(nbw, 1, c.Nout).astype(np.float64) if c.sw_rows else np.full((1, 1, 1), float(self.sw[0]))
        x1, x2 = split2(x, self.sx)
        w1, w2 = split2(w, self.sw.reshape(nbw, c.Nout, 1) if c.sw_rows else self.sw[0])
        self.Xp = pack(x1.reshape(-1, c.Kc), x2.reshape(-1, c.Kc), self.ldx)
        self.Wp = pack(w1.reshape(-1, self.K), w2.reshape(-1, self.K))
        self.factor = c.alpha / (float(self.sx) * swn)                                                 # [nbw | 1, 1, Nout | 1]
        # the lattice unit of the output: granularity of the plane products x |alpha| / (sx sw)
        self.gran = 1024.0 if c.rich else 4096.0
        self.unit = np.abs(self.factor) * self.gran * np.ones((1, 1, c.Nout))
        g = _rng(s + 2)
        if kind == "lattice":
            bias = (g.integers(-8, 9, c.Nout) * self.unit.max(axis=0)[0]) if c.bias else None          # a multiple of every item's unit
            out0 = (g.integers(-8, 9, (nb, self.M, c.Nout)) * self.unit) if c.beta else None
        else:
            bias = g.standard_normal(c.Nout) if c.bias else None
            out0 = g.standard_normal((nb, self.M, c.Nout)) if c.beta else None
        self.bias = None if bias is None else torch.from_numpy(bias.astype(F32))
        self.out0 = None if out0 is None else torch.from_numpy(out0.astype(F32))
        # gathered operands: true, plane 1, plane 2 in one gather
        t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
        stack = torch.cat([t(x), t(x1), t(x2)], dim=-1)                                                # [nb, xrows, 3 Kc]
        if taps == 1 and c.stride == 1 and c.pad == 0:
            A = stack.reshape(nb, self.M, 1, 3 * c.Kc)
        else:
            assert nb == 1
            gather = im2col if c.mode == 0 else im2col_dgrad
            A = gather(stack[0].reshape(c.N_img, c.Hi, c.Wi, 3 * c.Kc), c.KH, c.KW, c.stride, c.pad, c.dil, c.Ho, c.Wo)
            A = A.reshape(1, self.M, taps, 3 * c.Kc)
        self.A, self.A1, self.A2 = (A[..., i * c.Kc:(i + 1) * c.Kc].reshape(nb, self.M, self.K) for i in range(3))
        self.B, self.B1, self.B2 = (t(v).transpose(1, 2) for v in (w, w1, w2))                         # [nbw, K, Nout]
        self.chain = chain_h2(c.Kc, taps, c.nprod)
        self.build = h2_build(c)
        self._P = None

    def _products(self):
        if self._P is None:
            P, S = torch.matmul(self.A1, self.B1), torch.matmul(hw_abs(self.A1), hw_abs(self.B1))
            if self.c.nprod == 3:
                P = P + torch.matmul(self.A1, self.B2) + torch.matmul(self.A2, self.B1)
                S = S + torch.matmul(hw_abs(self.A1), hw_abs(self.B2)) + torch.matmul(hw_abs(self.A2), hw_abs(self.B1))
            self._P = (P, S)
        return self._P

    def _epilogue(self, acc, absolute=False):
        f = torch.from_numpy(np.abs(self.factor) if absolute else self.factor)
        r = acc * f
        for e in (self.bias, self.out0):
            if e is not None:
                r = r + (e.double().abs() if absolute else e.double())
        return r.clamp_min(0.0) if (self.c.relu and not absolute) else r

    def planes(self, drop=None, cross=None):
        """(R_planes, S).  drop: a k index left out of every product; cross: a K-tile whose a1 b2 is left out"""
        P, S = self._products()
        if drop is not None:
            k = slice(drop, drop + 1)
            P = P - torch.matmul(self.A1[..., k], self.B1[:, k])
            if self.c.nprod == 3:
                P = P - torch.matmul(self.A1[..., k], self.B2[:, k]) - torch.matmul(self.A2[..., k], self.B1[:, k])
        if cross is not None:
            k = slice(32 * cross, 32 * cross + 32)
            P = P - torch.matmul(self.A1[..., k], self.B2[:, k])
        return self._epilogue(P), self._epilogue(S, True)

    def true(self):
        """R_true: the contraction on the fp32 operands"""
        r = self.c.alpha * torch.matmul(self.A, self.B)
        for e in (self.bias, self.out0):
            if e is not None:
                r = r + e.double()
        return r.clamp_min(0.0) if self.c.relu else r

    def rep_bar(self):
        """|R_planes - R_true| <= this, element-wise"""
        sw = torch.from_numpy((self.c.alpha / (self.factor * float(self.sx))))                          # [.., 1, Nout | 1]: the weight scales
        absA, absB = self.A.abs() * float(self.sx), self.B.abs() * sw
        return rep_bound(absA, absB, self.c.nprod) * torch.from_numpy(np.abs(self.factor)) + 1e-13 * self.planes()[1] + 2.0 ** -149

    def exact_span(self):
        """largest S / unit: <= 2^24 guarantees that every fp32 summation order is exact (lattice data)"""
        return float((self.planes()[1] / torch.from_numpy(self.unit)).max())

    def last_live_k(self):
        """the last k that some output reads: its A column and its B row both hold a non-zero main plane"""
        live = ((self.A1 != 0).reshape(-1, self.K).any(0) & (self.B1 != 0).transpose(1, 2).reshape(-1, self.K).any(0)).nonzero()
        return int(live[-1])


# ====================================================================================================================
# weight gradient (hw_kernel, hw2_kernel) cases
# ====================================================================================================================
_HW = namedtuple("HWCase", "name N_img Hi Wi Ci Ho Wo Co KH KW stride pad dil alpha beta nbatch xvec yvec ldy_pad ldo_pad nprod rich")
_HW_DEF = dict(alpha=-0.5, beta=0, nbatch=1, xvec=False, yvec=False, ldy_pad=16, ldo_pad=4, nprod=3, rich=False)


def _wg(name, rows, Co, Ci, **kw):
    return _HW(name, rows, 1, 1, Ci, 1, 1, Co, 1, 1, 1, 0, 1, **{**_HW_DEF, **kw})


def _wc(name, N, H, W, Ci, Co, k, stride, pad, dil, **kw):
    return _HW(name, N, H, W, Ci, conv_out_size(H, k, stride, pad, dil), conv_out_size(W, k, stride, pad, dil), Co, k, k, stride, pad, dil,
               **{**_HW_DEF, **kw})


HW_ROWS = (1, 31, 32, 33, 257, 2049, 4100)
HW_CO = (16, 240, 256, 272)
HW_CI = (16, 112, 128, 144)


def hw_cases():
    cs = []
    for rows in HW_ROWS:
        cs.append(_wg(f"rows{rows}", rows, 272, 144, rich=rows <= 257))
    for Co in HW_CO:
        cs.append(_wg(f"Co{Co}", 33, Co, 144))
    for Ci in HW_CI:
        cs.append(_wg(f"Ci{Ci}", 33, 272, Ci))
    for beta in (0, 1):
        for alpha in (1.0, -0.5):
            cs.append(_wg(f"beta{beta}alpha{alpha}-direct", 257, 48, 32, alpha=alpha, beta=beta))
            cs.append(_wg(f"beta{beta}alpha{alpha}-slabs", 2049, 48, 32, alpha=alpha, beta=beta))
            cs.append(_wg(f"beta{beta}alpha{alpha}-slabs-ldo-odd", 2049, 48, 32, alpha=alpha, beta=beta, ldo_pad=1))      # hw_reduce_kernel
    for xvec in (False, True):
        for yvec in (False, True):
            cs.append(_wg(f"xvec{int(xvec)}yvec{int(yvec)}-direct", 257, 48, 32, xvec=xvec, yvec=yvec, beta=1))
            cs.append(_wg(f"xvec{int(xvec)}yvec{int(yvec)}-slabs", 2049, 48, 32, xvec=xvec, yvec=yvec))
            cs.append(_wg(f"xvec{int(xvec)}yvec{int(yvec)}-slabs-ldo-odd", 4100, 16, 16, xvec=xvec, yvec=yvec, ldo_pad=1, beta=1))
    cs.append(_wg("dense-ldy-ldo", 257, 48, 32, ldy_pad=0, ldo_pad=0))
    cs += [_wc(f"conv-3x3-Ci{Ci}", 2, 9, 13, Ci, 32, 3, 1, 1, 1, xvec=Ci == 32) for Ci in (16, 32, 48)]     # column tiles span several taps
    cs += [_wc("conv-3x3-stride2-dil2", 2, 9, 13, 32, 48, 3, 2, 2, 2, beta=1, yvec=True),
           _wc("conv-1x1-image-3x3", 3, 1, 1, 32, 16, 3, 1, 1, 1),
           _wc("conv-7x7-stride2", 2, 17, 21, 16, 32, 7, 2, 3, 1),
           _wc("conv-3x3-slabs", 3, 24, 32, 32, 48, 3, 1, 1, 1, beta=1, xvec=True, yvec=True)]               # 2304 pixels
    return cs


def hw_x1_cases():
    return [_wg("x1-rows33", 33, 272, 144, nprod=1), _wg("x1-rows257-beta1", 257, 48, 32, nprod=1, beta=1),
            _wg("x1-rows2049-slabs", 2049, 48, 32, nprod=1), _wg("x1-rows4100-slabs-ldo-odd", 4100, 16, 16, nprod=1, ldo_pad=1),
            _wc("x1-conv-3x3-Ci48", 2, 9, 13, 48, 32, 3, 1, 1, 1, nprod=1), _wc("x1-conv-3x3-slabs", 3, 24, 32, 32, 48, 3, 1, 1, 1, nprod=1, beta=1)]


def hw_batched_cases():
    """nbatch 3, Ci padded to 16: ldo 12 (< Ci: Nvalid = 12) and 20"""
    return [_wg(f"batch3-rows{rows}-ldo{ldo}-beta{beta}", rows, 48, 16, nbatch=3, ldo_pad=ldo - 16, beta=beta)
            for rows in (32, 96) for ldo in (12, 20) for beta in (0, 1)]


class HWProblem:
    def __init__(self, c, kind="gauss", seed_extra="", dy_mul=1.0, dead_rows=None, **lattice_kw):
        """dy_mul: a power of two on the gradient (the applications of sp_conv_wgrad_f16x2_multi); dead_rows: pixel rows whose gradient is exactly
        zero by the row_last contract -- zero in the reference, NaN planes in the operand (they must not be read)"""
        self.c, self.kind = c, kind
        s = seed_of("hw" + kind + c.name + seed_extra)
        taps, nb = c.KH * c.KW, c.nbatch
        self.M, self.Ntot = c.N_img * c.Ho * c.Wo, taps * c.Ci
        self.xrows = c.N_img * c.Hi * c.Wi
        self.ldy, self.ldo = c.Co + c.ldy_pad, self.Ntot + c.ldo_pad
        self.Nvalid = min(self.Ntot, self.ldo)
        x = make(kind, (nb, self.xrows, c.Ci), (2,) if c.xvec else (), s, c.rich, **lattice_kw)
        dy = make(kind, (nb, self.M, c.Co), (2,) if c.yvec else (), s + 1, c.rich, **lattice_kw) * F32(dy_mul)
        if nb > 1 and self.Nvalid < self.Ntot:
            x[..., self.Nvalid:] = 0                                                                    # the padding channels of a padded Ci
        self.x, self.dy = x, dy
        colscale = lambda v: np.array([scale_of(a) if a > 0 else F32(2.0 ** 100) for a in np.fmax.reduce(np.abs(v.reshape(-1, v.shape[-1])), axis=0)], F32)
        self.sx = colscale(x) if c.xvec else np.full(1, scale_of(_amax(x)), F32)
        self.sy = colscale(dy) if c.yvec else np.full(1, scale_of(_amax(dy)), F32)
        x1, x2 = split2(x, self.sx)
        y1, y2 = split2(dy, self.sy)
        self.Xp = pack(x1.reshape(-1, c.Ci), x2.reshape(-1, c.Ci))
        if dead_rows is not None:
            y1, y2, dy = y1.copy(), y2.copy(), dy.copy()
            y1.view(np.uint16)[:, dead_rows], y2.view(np.uint16)[:, dead_rows] = F16_NAN, F16_NAN
        self.Yp = pack(y1.reshape(-1, c.Co), y2.reshape(-1, c.Co), self.ldy)
        if dead_rows is not None:
            y1[:, dead_rows], y2[:, dead_rows], dy[:, dead_rows] = 0, 0, 0
        sxn = np.tile(self.sx.astype(np.float64), taps) if c.xvec else np.full(self.Ntot, float(self.sx[0]))
        syn = self.sy.astype(np.float64) if c.yvec else np.full(c.Co, float(self.sy[0]))
        self.sxn, self.syn = sxn, syn
        self.factor = (c.alpha / (syn[:, None] * sxn[None, :]))[None]                                   # [1, Co, Ntot]
        self.gran = 1024.0 if c.rich else 4096.0
        self.unit = np.abs(self.factor) * self.gran
        g = _rng(s + 2)
        if c.beta:
            out0 = g.integers(-8, 9, (nb, c.Co, self.Ntot)) * self.unit if kind == "lattice" else g.standard_normal((nb, c.Co, self.Ntot))
            self.out0 = torch.from_numpy(out0.astype(F32))
        else:
            self.out0 = None
        t = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float64))
        stack = torch.cat([t(x), t(x1), t(x2)], dim=-1)
        if taps == 1 and c.stride == 1 and c.pad == 0:
            Bm = stack.reshape(nb, self.M, 1, 3 * c.Ci)
        else:
            assert nb == 1
            Bm = im2col(stack[0].reshape(c.N_img, c.Hi, c.Wi, 3 * c.Ci), c.KH, c.KW, c.stride, c.pad, c.dil, c.Ho, c.Wo).reshape(1, self.M, taps, 3 * c.Ci)
        self.B, self.B1, self.B2 = (Bm[..., i * c.Ci:(i + 1) * c.Ci].reshape(nb, self.M, self.Ntot) for i in range(3))
        self.A, self.A1, self.A2 = (t(v).transpose(1, 2) for v in (dy, y1, y2))                         # [nb, Co, M]
        self.K = self.M
        self.splits = 1 if nb > 1 else hw_splits(self.M, c.Co, self.Ntot)
        self.chain = chain_hw(self.M, self.splits, c.nprod)
        self.reducer = hw_reducer(self.Ntot, self.ldo, c.Co, c.Ci) if self.splits > 1 else None
        self.build = f"hw<nprod{c.nprod}>" + (f"+{self.reducer}" if self.reducer else "") + ("+batched" if nb > 1 else "")
        self._P = None

    _products = H2Problem._products

    def _epilogue(self, acc, absolute=False):
        r = acc * torch.from_numpy(np.abs(self.factor) if absolute else self.factor)
        if self.out0 is not None:
            r = r + (self.out0.double().abs() if absolute else self.out0.double())
        return r

    def planes(self, drop=None, cross=None):
        P, S = self._products()
        if drop is not None:
            k = slice(drop, drop + 1)
            P = P - torch.matmul(self.A1[..., k], self.B1[:, k])
            if self.c.nprod == 3:
                P = P - torch.matmul(self.A1[..., k], self.B2[:, k]) - torch.matmul(self.A2[..., k], self.B1[:, k])
        if cross is not None:
            k = slice(32 * cross, 32 * cross + 32)
            P = P - torch.matmul(self.A1[..., k], self.B2[:, k])
        return self._epilogue(P), self._epilogue(S, True)

    def true(self):
        r = self.c.alpha * torch.matmul(self.A, self.B)
        return r if self.out0 is None else r + self.out0.double()

    def rep_bar(self):
        absA, absB = self.A.abs() * torch.from_numpy(self.syn)[None, :, None], self.B.abs() * torch.from_numpy(self.sxn)[None, None, :]
        return rep_bound(absA, absB, self.c.nprod) * torch.from_numpy(np.abs(self.factor)) + 1e-13 * self.planes()[1] + 2.0 ** -149

    def exact_span(self):
        return float((self.planes()[1] / torch.from_numpy(self.unit)).max())

    def last_live_k(self):
        live = ((self.A1 != 0).reshape(-1, self.K).any(0) & (self.B1 != 0).transpose(1, 2).reshape(-1, self.K).any(0)).nonzero()
        return int(live[-1])


def hw_desc(hip, p, **kw):
    """the sp_wgrad_desc of an HWProblem (hip: scanpaths_amd.hip); kw overrides fields"""
    c = p.c
    a = dict(N_img=c.N_img, Hi=c.Hi, Wi=c.Wi, Ci=c.Ci, ldx=c.Ci, Ho=c.Ho, Wo=c.Wo, Co=c.Co, ldy=p.ldy, KH=c.KH, KW=c.KW, stride=c.stride, pad=c.pad,
             dil=c.dil, ldo=p.ldo, beta=c.beta, alpha=c.alpha, nbatch=c.nbatch, x_scale_vec=int(c.xvec), y_scale_vec=int(c.yvec),
             strideX=p.xrows * c.Ci if c.nbatch > 1 else 0, strideY=p.M * p.ldy if c.nbatch > 1 else 0, strideO=c.Co * p.ldo if c.nbatch > 1 else 0)
    a.update(kw)
    return hip.WgradDesc(**a)
