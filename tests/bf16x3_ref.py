"""Plain restatement of the 3xbf16 kernels of csrc/conv_bf16x3.hip -- the two operand splitters bit for bit, and every GEMM launch as two fp64
contractions -- the reference side of tests/test_bf16x3_ref_cpu.py and tests/test_conv_bf16x3_gpu.py.  Nothing here touches a GPU.

OPERANDS.  x1 = bf16(x), x2 = bf16(x - x1), x3 = bf16(x - x1 - x2), round to nearest even, both residuals exact in fp32 (split3), stored as
[row][K / 16][plane][16] bf16 followed by a 64-byte zero block (pack3).  sp_split3_bf16 takes the rows as they come, sp_split3_bf16_wT turns
w [Co][taps][Ci] into rows ci with k = (tap, co).  For a normal fp32 x whose planes stay normal (|x| >= 2^-100 is ample: plane 3 is a multiple
of ulp(x) >= 2^-123) x1 + x2 + x3 == x EXACTLY -- three 8-bit significands cover the 24 bits of x (test_bf16x3_ref_cpu.py: 2^20 values across
2^+-30, residual 0).  An infinite or NaN x gives (x, NaN, NaN): inf - inf is NaN; a finite x that rounds past the largest bf16 gives
(+-inf, -+inf, NaN).  This states the rule; nothing changes it.  Every case here keeps |x| >= 2^-100 or x = 0; subnormal planes
(f16x2_ref.hw_abs says why they need a bar of their own) are not exercised.

TWO CONTRACTIONS PER LAUNCH, both in fp64:
    R_planes   what the kernel is asked to compute: the decoded planes with exactly the SIX products it takes -- a1b3, a3b1, a2b2, a1b2, a2b1,
               a1b1; never a2b3, a3b2, a3b3 -- then the epilogue of the ABI (igemm: alpha, bias, beta out, relu; wgrad: alpha, beta out)
    R_true     the same contraction on the fp32 operands
The gathers are gemm_ref.im2col / im2col_dgrad; the weight operand is always [Nout][K] with k = (tap, channel).

TWO BARS, both derived, neither tuned on results:
    kernel against R_planes   parity.bar(S, c): c 2^-24 S + 2^-149, S the contraction over absolute plane values (the same six products), c the
                              launch's longest chain of dependent roundings in units of 2^-24 (chain_b3, chain_w3).
                              ASSUMPTION, the one f16x2_ref.PROD_UNITS states for v_mfma_f32_16x16x32_f16, taken over unchanged: nobody here has
                              measured what one v_mfma_f32_32x32x16_bf16 does internally.  bf16 x bf16 products are exact in fp32 (16
                              significand bits), and every product of the 16 an instruction adds into its accumulator costs at most ONE
                              TRUNCATION, 2^-23 = PROD_UNITS units.  A K-tile is six such instructions into the same accumulator.
    R_planes against R_true   rep_bound: the three dropped products and the splitter's residual, derived there (about 2^-25 |a||b|).

LATTICE DATA.  An entry is 0, a UNIT +-1 (planes +-1, 0, 0) or a FULL value +-5 +- 3 2^-8 (+- 2^-16): small integers times 2^0, 2^-8, 2^-16,
chosen inside their binades (5 in [4, 8), 3 in [2, 4)) so that every residual stays below half an ulp of the plane above it and the restated
splitter returns exactly these planes (asserted where the data is made).  Every product of the six is then a multiple of 2^-16, and while
S / 2^-16 <= 2^24 every fp32 summation order gives the bits of the fp64 sum; alpha a power of two, bias / out0 on the output's lattice: the
kernel must equal R_planes WORD FOR WORD.  A product of two full values costs 25 of the 256 units of S that condition allows, so K is limited
(to roughly 64 with mixed entries); long contractions use SPARSE non-zeros placed so that every K-tile still reaches some output (igemm: one
non-zero per pixel and 16-channel block against weight blocks thinned to about twelve per output; wgrad: one non-zero channel per pixel on both
sides, so every pixel lands in exactly one output word per tap) -- a dropped, repeated, stale or misplaced K-tile changes an exact word."""
from collections import namedtuple

import numpy as np
import torch

from f16x2_ref import PROD_UNITS
from gemm_ref import conv_out_size, im2col, im2col_dgrad
from parity import U, cdiv, seed_of

F32 = np.float32
CHUNK_KT = 16           # K-tiles between two folds of `acc` into `tot` (b3_kernel and w3_kernel)
KT_PRODUCTS = 6 * 16    # products one K-tile adds into one accumulator word: six instructions of 16 k
LATTICE_UNIT = 2.0 ** -16
BF16_QNAN = 0x7FC0


# ====================================================================================================================
# (a) the splitters, bit for bit
# ====================================================================================================================
def bf16_bits(x):
    """fp32 -> bf16 bits, round to nearest even (a NaN stays a NaN, quiet; a value past the largest bf16 becomes an infinity)"""
    x = np.ascontiguousarray(x, dtype=F32)
    u = x.view(np.uint32).astype(np.uint64)
    out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    nan = np.isnan(x)
    if nan.any():
        out[nan] = ((u[nan] >> 16) | 0x40).astype(np.uint16)
    return out


def bf16_value(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(F32)


def split3(v):
    """split3 of conv_bf16x3.hip, element-wise: three uint16 arrays of v's shape"""
    v = np.ascontiguousarray(v, dtype=F32)
    with np.errstate(invalid="ignore", over="ignore"):
        x1 = bf16_bits(v)
        r1 = (v - bf16_value(x1)).astype(F32)
        x2 = bf16_bits(r1)
        r2 = (r1 - bf16_value(x2)).astype(F32)
        x3 = bf16_bits(r2)
    return x1, x2, x3


def decode3(x1, x2, x3):
    """the fp64 value of three planes (each sum below is exact: the planes of one fp32 number span at most 53 bits for |x| >= 2^-100)"""
    return bf16_value(x1).astype(np.float64) + bf16_value(x2).astype(np.float64) + bf16_value(x3).astype(np.float64)


def pack3(x1, x2, x3):
    """[rows][K] planes -> uint16 [rows][K / 16][3][16] + 32 zero halves (the 64-byte zero block)"""
    rows, K = x1.shape
    assert K % 16 == 0
    out = np.stack([x1, x2, x3]).reshape(3, rows, K // 16, 16).transpose(1, 2, 0, 3)
    return np.concatenate([out.reshape(-1), np.zeros(32, np.uint16)])


def unpack3(buf, rows, K):
    """the inverse of pack3: three fp64 arrays [rows][K]"""
    p = bf16_value(np.asarray(buf[:3 * rows * K], dtype=np.uint16)).astype(np.float64).reshape(rows, K // 16, 3, 16)
    return tuple(p[:, :, i].reshape(rows, K) for i in range(3))


def split3_bf16(x):
    """sp_split3_bf16: x fp32 [n], n % 16 == 0 (rows are whole 16-groups, so the flat order is the layout)"""
    x = np.asarray(x, dtype=F32).reshape(1, -1)
    return pack3(*split3(x))


def split3_bf16_wT(w):
    """sp_split3_bf16_wT: w [Co][taps][Ci] -> rows ci, k = (tap, co)"""
    w = np.asarray(w, dtype=F32)
    Co, taps, Ci = w.shape
    return pack3(*split3(np.ascontiguousarray(w.transpose(2, 1, 0)).reshape(Ci, taps * Co)))


# ====================================================================================================================
# (b) chains of dependent roundings, in units of 2^-24, and the plans
# ====================================================================================================================
def _chain(n):
    """(1 + u)^n - 1 <= n u (1 + 2 n u) while n u <= 1/2; plus one unit for the fp64 reference's own error"""
    assert n * U <= 0.5
    return int(np.ceil(n * (1 + 2 * n * U))) + 1


def chain_b3(Kc, taps):
    """b3_kernel: a K-tile is 6 v_mfma_f32_32x32x16_bf16 of 16 k into ONE accumulator: 96 products of PROD_UNITS each, at most CHUNK_KT = 16
    tiles before `acc` is folded into `tot` (fold: (kt & 15) == 15) and restarted; one add per fold, nkt // 16 folds and the epilogue's
    tot + acc; the epilogue multiplies by alpha and adds bias and out: 3."""
    nkt = taps * Kc // 16
    return _chain(PROD_UNITS * KT_PRODUCTS * min(CHUNK_KT, nkt) + (nkt // CHUNK_KT + 1) + 3)


def w3_splits(M, Co, Ntot):
    """w3_splits of the launcher: 2048 / tiles workgroups wanted, at least 512 pixels (32 K-tiles) per split, at most 64 splits"""
    tiles = cdiv(Co, 256) * cdiv(Ntot, 128)
    return max(1, min(cdiv(2048, tiles), max(1, M // 512), 64))


def rows_per_split(M, splits):
    return cdiv(cdiv(M, splits), 16) * 16


def w3_workspace(M, Co, Ntot, ldo):
    s = w3_splits(M, Co, Ntot)
    return 0 if s <= 1 else s * Co * ldo * 4


def chain_w3(M, splits):
    """w3_kernel + wgrad3_reduce_kernel: per split the chain of b3_kernel over rows_per_split / 16 K-tiles of 16 pixels.  Direct (one split):
    alpha, beta out: 2.  Through slabs: the reducer adds the `splits` slabs onto 0.f, multiplies by alpha, adds out: splits + 2."""
    nkt = cdiv(min(M, rows_per_split(M, splits)), 16)
    return _chain(PROD_UNITS * KT_PRODUCTS * min(CHUNK_KT, nkt) + (nkt // CHUNK_KT + 1) + (2 if splits <= 1 else splits + 2))


def w3_walk(Ho, Wo, nkt, m_begin=0, fixed=True):
    """the (image, y, x) of loader lane r = 0 .. 15 at the K-tiles 0 .. nkt - 1 of w3_kernel, by ITS rule: coordinates of pixel m_begin + r by
    division, then per K-tile x += 16 % Wo, y += 16 // Wo, one wrap of x, one wrap of y -- and, fixed, on maps of fewer than 16 pixels further
    wraps of y while it is past the map (the parent's kernel had the single `if` alone).  [nkt, 16, 3]"""
    y_adv, x_adv = 16 // Wo, 16 - (16 // Wo) * Wo
    tiny = Ho * Wo < 16
    out = np.zeros((nkt, 16, 3), np.int64)
    for r in range(16):
        m = m_begin + r
        b, rem = divmod(m, Ho * Wo)
        y, x = divmod(rem, Wo)
        for kt in range(nkt):
            out[kt, r] = (b, y, x)
            x += x_adv
            y += y_adv
            if x >= Wo:
                x -= Wo
                y += 1
            if y >= Ho:
                y -= Ho
                b += 1
            if fixed and tiny:
                while y >= Ho:
                    y -= Ho
                    b += 1
    return out


def w3_walk_true(Ho, Wo, nkt, m_begin=0):
    m = m_begin + 16 * np.arange(nkt)[:, None] + np.arange(16)[None, :]
    return np.stack([m // (Ho * Wo), (m % (Ho * Wo)) // Wo, m % Wo], axis=-1)


# ====================================================================================================================
# (c) the representation bound
# ====================================================================================================================
def rep_bound(absA, absB):
    """|sum_k a b - (the six products)| element-wise ([.., M, K] x [.., K, N], fp64 absolute values of the fp32 operands, no plane subnormal).
    h = 2^-9 (bf16 round to nearest): a = a1 + a2 + a3 + ea with |a - a1| <= h |a|, |a2| <= d2 |a|, d2 = h (1 + h), |a - a1 - a2| <= h^2 |a|,
    |a3| <= d3 |a|, d3 = h^2 (1 + h), |ea| <= h^3 |a| (it is in fact 0: exact decode).  Then
        a b - six = a2 b3 + a3 b2 + a3 b3 + ea b + (a - ea) eb  <=  (2 d2 d3 + d3^2 + h^3 (2 + h^3)) |a| |b|  ~  4 x 2^-27 |a b| = 2^-25 |a b|"""
    h = 2.0 ** -9
    d2, d3 = h * (1 + h), h * h * (1 + h)
    return (2 * d2 * d3 + d3 * d3 + h ** 3 * (2 + h ** 3)) * torch.matmul(absA, absB)


# ====================================================================================================================
# data
# ====================================================================================================================
def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def gauss(shape, seed):
    x = _rng(seed).standard_normal(shape).astype(F32)
    assert (np.abs(x) >= 2.0 ** -100).all()
    return x


def heavy(shape, seed):
    """heavy-tailed gradients: randn * rand^4, kept at or above 2^-100 in magnitude"""
    g = _rng(seed)
    x = (g.standard_normal(shape) * g.random(shape) ** 4).astype(F32)
    x[np.abs(x) < 2.0 ** -100] = 0
    return x


def wide(n, seed):
    """normal values across 2^+-30"""
    g = _rng(seed)
    return (g.standard_normal(n) * np.exp2(g.uniform(-30, 30, n))).astype(F32)


def lattice_values(mask, seed, full_share=0.25):
    """(x fp32, (P1, P2, P3) fp64): non-zero where mask; a quarter FULL +-5 +- 3 2^-8 (+- 2^-16, three in four), the rest UNITS +-1.  Asserts
    that split3 returns exactly the intended planes."""
    g = _rng(seed)
    shape = mask.shape
    sign = lambda: g.choice([-1.0, 1.0], shape)
    full = mask & (g.random(shape) < full_share)
    unit = mask & ~full
    P1 = 5.0 * sign() * full + sign() * unit
    P2 = 3.0 * sign() * full * 2.0 ** -8
    P3 = sign() * (full & (g.random(shape) < 0.75)) * 2.0 ** -16
    x = (P1 + P2 + P3).astype(F32)
    assert (x.astype(np.float64) == P1 + P2 + P3).all()
    got = split3(x)
    for want, have in zip((P1, P2, P3), got):
        assert (bf16_value(have).astype(np.float64) == want).all(), "the splitter does not return the lattice's planes"
    return x, (P1, P2, P3)


def one_per_group(shape, group, seed, keep=1.0):
    """a mask with exactly one True per `group` consecutive entries of the last axis (w.p. keep per group)"""
    g = _rng(seed)
    n = int(np.prod(shape)) // group
    m = np.zeros((n, group), bool)
    m[np.arange(n), g.integers(0, group, n)] = g.random(n) < keep
    return m.reshape(shape)


def group_mask(shape, group, seed, keep):
    """whole groups of `group` consecutive entries of the last axis, each kept w.p. keep"""
    g = _rng(seed)
    n = int(np.prod(shape)) // group
    return np.repeat(g.random(n) < keep, group).reshape(shape)


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _six(A, B, absolute=False):
    """the six products: a1 (b1 + b2 + b3) + a2 (b1 + b2) + a3 b1 -- the inner sums are exact in fp64"""
    if absolute:
        A, B = [a.abs() for a in A], [b.abs() for b in B]
    return torch.matmul(A[0], B[0] + B[1] + B[2]) + torch.matmul(A[1], B[0] + B[1]) + torch.matmul(A[2], B[0])


def six_naive(A, B):
    """the same, product by product in the kernel's order (tiny cases only)"""
    M, K = A[0].shape
    N = B[0].shape[1]
    out = torch.zeros(M, N, dtype=torch.float64)
    for (i, j) in ((0, 2), (2, 0), (1, 1), (0, 1), (1, 0), (0, 0)):
        for m in range(M):
            for n in range(N):
                for k in range(K):
                    out[m, n] += A[i][m, k] * B[j][k, n]
    return out


class _Problem:
    """what the two problems share: the epilogue, the two restatements and the bars"""
    def planes(self):
        """(R_planes, S)"""
        if self._P is None:
            self._P = (self._epilogue(_six(self.Ap, self.Bp)), self._epilogue(_six(self.Ap, self.Bp, True), True))
        return self._P

    def true(self):
        return self._epilogue(torch.matmul(self.A, self.B))

    def rep_bar(self):
        """|R_planes - R_true| <= this, element-wise (relu is a contraction: it cannot widen the difference)"""
        return abs(self.alpha) * rep_bound(self.A.abs(), self.B.abs()) + 1e-13 * self.planes()[1] + 2.0 ** -149

    def exact_span(self):
        """S in units of the output's lattice: <= 2^24 makes every fp32 order exact"""
        return float(self.planes()[1].max()) / (abs(self.alpha) * LATTICE_UNIT)

    def _extras(self, kind, seed, shape_bias, shape_out, want_bias, want_out):
        g = _rng(seed)
        u = abs(self.alpha) * LATTICE_UNIT
        mk = (lambda s: g.integers(-8, 9, s) * u) if kind == "lattice" else (lambda s: g.standard_normal(s))
        bias = mk(shape_bias) if want_bias else None
        out0 = mk(shape_out) if want_out else None
        self.bias = None if bias is None else torch.from_numpy(bias.astype(F32))
        self.out0 = None if out0 is None else torch.from_numpy(out0.astype(F32))


# ====================================================================================================================
# igemm (b3_kernel) cases
# ====================================================================================================================
_B3 = namedtuple("B3Case", "name N_img Hi Wi Kc Ho Wo Nout KH KW stride pad dil mode alpha bias beta relu ldc_pad")
_B3_DEF = dict(alpha=-0.5, bias=True, beta=0, relu=False, ldc_pad=3)


def _bg(name, M, Kc, Nout, mode, **kw):
    return _B3(name, M, 1, 1, Kc, 1, 1, Nout, 1, 1, 1, 0, 1, mode, **{**_B3_DEF, **kw})


def _bc(name, N, H, W, Kc, Nout, k, stride, pad, dil, mode, **kw):
    """a conv case by the CONV's input size: mode 0 computes the conv, mode 1 its input gradient (the launch's Ho x Wo = H x W)"""
    h, w = conv_out_size(H, k, stride, pad, dil), conv_out_size(W, k, stride, pad, dil)
    a = {**_B3_DEF, **kw}
    if mode == 0:
        return _B3(name, N, H, W, Kc, h, w, Nout, k, k, stride, pad, dil, 0, **a)
    return _B3(name, N, h, w, Kc, H, W, Nout, k, k, stride, pad, dil, 1, **a)


B3_NKT = (1, 2, 3, 4, 5, 15, 16, 17, 32, 33)      # every branch of the counted vmcnt in prologue and loop, the fold at 16, a remainder after it
B3_M = (1, 255, 256, 257, 513)
B3_NOUT = (1, 127, 128, 129, 260)


def b3_gemm_cases():
    cs = []
    for mode in (0, 1):
        m = f"mode{mode}"
        for nkt in B3_NKT:                          # Kc 16, 48, 64, 80 are the 1, 3, 4, 5 of this sweep
            cs.append(_bg(f"{m}-nkt{nkt}-Kc{16 * nkt}", 257, 16 * nkt, 129, mode))
        for M in B3_M:
            cs.append(_bg(f"{m}-M{M}", M, 64, 129, mode))
        for N in B3_NOUT:
            cs.append(_bg(f"{m}-Nout{N}", 257, 48, N, mode, ldc_pad=4 if N % 2 == 0 else 3))
    cs.append(_bg("mode1-Kc16-Nout4", 257, 16, 4, 1, ldc_pad=4))
    cs.append(_bg("mode1-Kc48-Nout130", 257, 48, 130, 1, ldc_pad=2))
    cs.append(_bg("mode0-supertile-4x8", 1024, 16, 1024, 0, ldc_pad=0, bias=False))
    cs.append(_bg("mode1-supertile-4x8", 1024, 16, 1024, 1, ldc_pad=4))
    cs.append(_bg("mode0-n-fastest-4x7", 1024, 16, 896, 0, ldc_pad=4))
    return cs


def b3_epilogue_cases():
    cs = []
    for bias in (False, True):
        for beta in (0, 1):
            for relu in (False, True):
                e = f"bias{int(bias)}beta{beta}relu{int(relu)}"
                cs.append(_bg(f"{e}-direct-nkt3", 257, 48, 129, 0, bias=bias, beta=beta, relu=relu))
                cs.append(_bg(f"{e}-folds-nkt17", 257, 272, 129, 0, bias=bias, beta=beta, relu=relu))
    return cs


def b3_conv_cases():
    cs = []
    for mode in (0, 1):
        m = f"mode{mode}"
        cs += [_bc(f"{m}-3x3-pad1-3-images-5x7-Kc16", 3, 5, 7, 16, 132, 3, 1, 1, 1, mode),          # image and padding edges inside one 256-row tile
               _bc(f"{m}-3x3-pad1-3-images-5x7-Kc48", 3, 5, 7, 48, 60, 3, 1, 1, 1, mode, ldc_pad=4, relu=True),
               _bc(f"{m}-3x3-pad1-9-images-5x7-Kc64", 9, 5, 7, 64, 130, 3, 1, 1, 1, mode, beta=1),    # 315 rows: two M-tiles, 36 K-tiles
               _bc(f"{m}-3x3-stride2-odd-9x13", 2, 9, 13, 16, 64, 3, 2, 1, 1, mode),
               _bc(f"{m}-3x3-stride2-even-8x12", 2, 8, 12, 48, 4, 3, 2, 1, 1, mode, ldc_pad=4),
               _bc(f"{m}-3x3-dil2-pad2-9x13", 2, 9, 13, 16, 64, 3, 1, 2, 2, mode),
               _bc(f"{m}-3x3-stride2-dil2-9x13", 1, 9, 13, 80, 130, 3, 2, 2, 2, mode, relu=True),
               _bc(f"{m}-7x7-stride2-pad3-Kc16", 1, 9, 13, 16, 64, 7, 2, 3, 1, mode),
               _bc(f"{m}-1x1-image-3x3", 2, 1, 1, 16, 64, 3, 1, 1, 1, mode)]
    return cs


class B3Problem(_Problem):
    """operands of an igemm case as fp32 arrays in the layout the device splitters take, the packed planes they must produce, and the two fp64
    restatements.  kind: gauss / heavy / lattice"""
    def __init__(self, c, kind="gauss"):
        self.c, self.kind, self.alpha = c, kind, c.alpha
        s = seed_of("b3" + kind + c.name)
        taps = c.KH * c.KW
        self.K, self.M, self.xrows, self.ldc = taps * c.Kc, c.N_img * c.Ho * c.Wo, c.N_img * c.Hi * c.Wi, c.Nout + c.ldc_pad
        nkt = self.K // 16
        if kind == "lattice":
            x, xp = lattice_values(one_per_group((self.xrows, c.Kc), 16, s), s + 10)
            w, wp = lattice_values(group_mask((c.Nout, taps, c.Kc), 16, s + 1, min(1.0, 12.0 / nkt)), s + 11)       # [Nout][tap][c]
        else:
            make = gauss if kind == "gauss" else heavy
            x, w = make((self.xrows, c.Kc), s), make((c.Nout, taps, c.Kc), s + 1)
            xp, wp = [bf16_value(p).astype(np.float64) for p in split3(x)], [bf16_value(p).astype(np.float64) for p in split3(w)]
        self.x = x
        self.Xp = split3_bf16(x)
        if c.mode == 0:
            self.w = w                                                                     # sp_split3_bf16 on [Nout][K]
            self.Wp = split3_bf16(w)
        else:
            self.w = np.ascontiguousarray(w.transpose(2, 1, 0))                            # the conv's weight [Co = Kc][taps][Ci = Nout]
            self.Wp = split3_bf16_wT(self.w)
        self._extras(kind, s + 2, c.Nout, (1, self.M, c.Nout), c.bias, c.beta)
        stack = torch.cat([_t(x)] + [_t(p) for p in xp], dim=-1)                           # [xrows, 4 Kc]
        if taps == 1 and c.stride == 1 and c.pad == 0:
            A = stack.reshape(self.M, 1, 4 * c.Kc)
        else:
            gather = im2col if c.mode == 0 else im2col_dgrad
            A = gather(stack.reshape(c.N_img, c.Hi, c.Wi, 4 * c.Kc), c.KH, c.KW, c.stride, c.pad, c.dil, c.Ho, c.Wo).reshape(self.M, taps, 4 * c.Kc)
        parts = [A[..., i * c.Kc:(i + 1) * c.Kc].reshape(1, self.M, self.K) for i in range(4)]
        self.A, self.Ap = parts[0], parts[1:]
        self.B = _t(w).reshape(1, c.Nout, self.K).transpose(1, 2)
        self.Bp = [_t(p).reshape(1, c.Nout, self.K).transpose(1, 2) for p in wp]
        self.chain = chain_b3(c.Kc, taps)
        self._P = None
        if kind == "lattice":
            assert self.exact_span() <= 2.0 ** 24, (c.name, self.exact_span())

    def _epilogue(self, acc, absolute=False):
        r = (abs(self.alpha) if absolute else self.alpha) * acc
        for e in (self.bias, self.out0):
            if e is not None:
                r = r + (e.double().abs() if absolute else e.double())
        return r.clamp_min(0.0) if (self.c.relu and not absolute) else r

    def live_tiles(self):
        """the share of K-tiles that some output reads through non-zero main planes"""
        a = (self.Ap[0] != 0).reshape(-1, self.K // 16, 16).any(0)
        b = (self.Bp[0] != 0).transpose(1, 2).reshape(-1, self.K // 16, 16).any(0)
        return float((a & b).any(-1).double().mean())


# ====================================================================================================================
# weight gradient (w3_kernel, wgrad3_reduce_kernel) cases
# ====================================================================================================================
_W3 = namedtuple("W3Case", "name N_img Hi Wi Ci Ho Wo Co KH KW stride pad dil alpha beta ldo_pad")
_W3_DEF = dict(alpha=-0.5, beta=0, ldo_pad=4)


def _wg(name, rows, Co, Ci, **kw):
    return _W3(name, rows, 1, 1, Ci, 1, 1, Co, 1, 1, 1, 0, 1, **{**_W3_DEF, **kw})


def _wc(name, N, H, W, Ci, Co, k, stride, pad, dil, **kw):
    return _W3(name, N, H, W, Ci, conv_out_size(H, k, stride, pad, dil), conv_out_size(W, k, stride, pad, dil), Co, k, k, stride, pad, dil,
               **{**_W3_DEF, **kw})


W3_ROWS = (1, 15, 16, 17, 33, 511, 512, 1023)
W3_CO = (16, 48, 240, 256, 272)
W3_SMALL_MAPS = ((2, 2), (3, 3), (3, 5), (1, 15), (7, 2))        # fewer than 16 pixels: the parent's one-`if` advance goes wrong
W3_MAPS = W3_SMALL_MAPS + ((4, 4), (1, 17), (5, 16))


def w3_gemm_cases():
    """Ho = Wo = 1: the pure-GEMM form of functional._gemm_wgrad_desc.  Every one with more than 16 rows fails on the parent's kernel."""
    cs = [_wg(f"rows{rows}", rows, 48, 128, beta=rows % 2) for rows in W3_ROWS]
    cs += [_wg(f"Co{Co}", 33, Co, 128) for Co in W3_CO]
    cs += [_wg("Ci256", 33, 16, 256, beta=1), _wg("Ci256-Co272", 17, 272, 256)]
    return cs


def w3_map_cases():
    cs = []
    for (H, W) in W3_MAPS:
        N = max(3, cdiv(70, H * W))                                                     # K-tiles cross several images
        cs.append(_wc(f"map-{H}x{W}-1x1-N{N}", N, H, W, 128, 16, 1, 1, 0, 1, beta=(H + W) % 2))
    for (H, W) in ((2, 2), (3, 3), (3, 5), (4, 4)):
        cs.append(_wc(f"map-{H}x{W}-3x3-pad1-N7", 7, H, W, 128, 48, 3, 1, 1, 1))
    cs += [_wc("3x3-pad1-9x13", 2, 9, 13, 128, 48, 3, 1, 1, 1, beta=1),
           _wc("3x3-stride2-5x7-to-3x4", 5, 5, 7, 128, 16, 3, 2, 1, 1),                     # a 12-pixel output map under stride 2
           _wc("3x3-stride2-9x13", 2, 9, 13, 128, 272, 3, 2, 1, 1),
           _wc("3x3-dil2-pad2-9x13", 2, 9, 13, 256, 16, 3, 1, 2, 2, beta=1),
           _wc("3x3-dil2-pad2-3x3", 6, 3, 3, 128, 16, 3, 1, 2, 2)]
    return cs


def w3_split_cases():
    """the edges of w3_splits at one tile (Co 16, Ci 128): 2 splits, a ragged last split, 3 splits; conv maps through slabs; the cap of 64"""
    cs = []
    for beta in (0, 1):
        cs.append(_wg(f"direct-rows257-beta{beta}", 257, 48, 128, beta=beta))
        cs.append(_wg(f"splits2-rows1024-beta{beta}", 1024, 16, 128, beta=beta))
    cs += [_wg("splits2-rows1025-ragged", 1025, 16, 128), _wg("splits2-rows1040-ragged", 1040, 16, 128, beta=1),
           _wg("splits3-rows1537", 1537, 16, 128), _wg("splits2-two-tiles-Co272", 1100, 272, 128, beta=1),
           _wc("splits2-map-3x3-N120", 120, 3, 3, 128, 16, 1, 1, 0, 1), _wc("splits2-3x3-pad1-24x45", 1, 24, 45, 128, 16, 3, 1, 1, 1, beta=1)]
    return cs


W3_CAP = _wg("splits64-rows32768", 32768, 16, 128, beta=1)


class W3Problem(_Problem):
    def __init__(self, c, kind="gauss"):
        self.c, self.kind, self.alpha = c, kind, c.alpha
        s = seed_of("w3" + kind + c.name)
        taps = c.KH * c.KW
        self.M, self.Ntot, self.xrows = c.N_img * c.Ho * c.Wo, taps * c.Ci, c.N_img * c.Hi * c.Wi
        self.K, self.ldo = self.M, taps * c.Ci + c.ldo_pad
        if kind == "lattice":
            x, xp = lattice_values(one_per_group((self.xrows, c.Ci), c.Ci, s), s + 10)
            dy, yp = lattice_values(one_per_group((self.M, c.Co), c.Co, s + 1, min(1.0, 12.0 * c.Co * c.Ci / self.M)), s + 11)
        else:
            make = gauss if kind == "gauss" else heavy
            x, dy = make((self.xrows, c.Ci), s), make((self.M, c.Co), s + 1)
            xp, yp = [bf16_value(p).astype(np.float64) for p in split3(x)], [bf16_value(p).astype(np.float64) for p in split3(dy)]
        self.x, self.dy = x, dy
        self.Xp, self.Yp = split3_bf16(x), split3_bf16(dy)
        self._extras(kind, s + 2, 0, (1, c.Co, self.Ntot), False, c.beta)
        stack = torch.cat([_t(x)] + [_t(p) for p in xp], dim=-1)
        if taps == 1 and c.stride == 1 and c.pad == 0:
            Bm = stack.reshape(self.M, 1, 4 * c.Ci)
        else:
            Bm = im2col(stack.reshape(c.N_img, c.Hi, c.Wi, 4 * c.Ci), c.KH, c.KW, c.stride, c.pad, c.dil, c.Ho, c.Wo).reshape(self.M, taps, 4 * c.Ci)
        parts = [Bm[..., i * c.Ci:(i + 1) * c.Ci].reshape(1, self.M, self.Ntot) for i in range(4)]
        self.B, self.Bp = parts[0], parts[1:]
        self.A = _t(dy).reshape(1, self.M, c.Co).transpose(1, 2)
        self.Ap = [_t(p).reshape(1, self.M, c.Co).transpose(1, 2) for p in yp]
        self.splits = w3_splits(self.M, c.Co, self.Ntot)
        self.chain = chain_w3(self.M, self.splits)
        self._P = None
        if kind == "lattice":
            assert self.exact_span() <= 2.0 ** 24, (c.name, self.exact_span())

    def _epilogue(self, acc, absolute=False):
        r = (abs(self.alpha) if absolute else self.alpha) * acc
        if self.out0 is not None:
            r = r + (self.out0.double().abs() if absolute else self.out0.double())
        return r

    def live_tiles(self):
        """the share of 16-pixel K-tiles that some output reads through non-zero main planes"""
        live = (self.Ap[0] != 0).reshape(-1, self.M).any(0) & (self.Bp[0] != 0).reshape(self.M, -1).any(1)
        pad = (-self.M) % 16
        return float(torch.cat([live, torch.zeros(pad, dtype=torch.bool)]).reshape(-1, 16).any(1).double().mean())
