"""Plain fp64 restatements, case tables and bars of the pooling, layout, column-sum and fan-in entry points of csrc/bn_pool.hip -- sp_maxpool3s2_fwd /
bwd, sp_colsum (+ its workspace query), sp_sum_n, sp_sum_n_mixed, sp_nchw_to_nhwc_pad, sp_pad_lastdim, sp_add, sp_relu_bwd: the reference side of
tests/test_pool_sum_ref_cpu.py and tests/test_pool_sum_gpu.py.  Nothing here touches a GPU and pytest collects nothing from it.

POOLING.  MaxPool2d(3, stride 2, pad 0, ceil_mode=True) on NHWC: Ho = ceil((H - 3) / 2) + 1, windows clipped at the lower / right edge.  The kernel's
rule is ATen's `(val > max) || isnan(val)` in row-major window order starting from (-inf, position 0): the FIRST maximum, a window holding only -inf
gives (-inf, 0), a NaN makes the output NaN at the window's LAST NaN.  The position byte is ky * 3 + kx.  Values and bytes are EXACT.  The backward
gathers, per input element, the dy of the (at most four) windows whose byte names it, in (oy, ox) order, in fp32 from 0: three roundings, c = 4, S the
same gather over |dy|.

SUMS.  sp_colsum, sp_sum_n and sp_sum_n_mixed add k terms in fp64 and round to fp32 ONCE:
    |got - ref| <= 2^-24 |ref| + k 2^-53 S + 2^-149             (S: the sum over absolute values)
= parity.bar(S', 1) with S' = |ref| + k 2^-29 S (rounded_once).  The first term is measured against |ref|, NOT against S: on cancelling data (terms of
1e4 that leave 1e-3) an fp32 accumulation misses it by many orders (f32_in_order, held to >= 100x by the CPU module), and that is what makes the
fp64 accumulation testable.  k 2^-53 S covers the k fp64 adds (each rounds at 2^-53 of a partial sum <= S).  sp_colsum with beta = 1 adds fp32(s) to
the old output in fp32, a second rounding: 2^-24 (|s| + |ref|) + k 2^-53 S + 2^-149 (rounded_twice).  No figure here was measured on a kernel.

LATTICE DATA: integers -3 .. 3 times a power of two, S / unit <= 2^24, so every partial sum in every order and format is exact and the result equals
the fp64 sum word for word (Summary.exact).  Under that condition an fp32 accumulation is exact too -- no such case can tell the two apart.  The
WIDE lattice (terms +A, small, -A with A = 2^26 units) is the case that does: S / unit <= 2^53 keeps every fp64 partial sum exact, |ref| / unit <= 2^24
keeps the result representable, and fp32 partial sums lose the small terms."""
import itertools
from collections import namedtuple

import numpy as np

from parity import cdiv, seed_of

F32, F64, F16 = np.float32, np.float64, np.float16
EW_BLOCK = 256                       # threads per block of every grid-stride kernel here
EW_CAP = 2048                        # sp_ew_grid cap of the element-wise launches (the pooling backward: 4 x 2048)


def rng(name):
    return np.random.Generator(np.random.PCG64(seed_of(name)))


def rounded_once(ref, S, k):
    """S' with parity.bar(S', 1) = 2^-24 |ref| + k 2^-53 S + 2^-149"""
    return np.abs(ref) + k * 2.0 ** -29 * S


def rounded_twice(s, ref, S, k):
    """sp_colsum with beta = 1: fp32(s) and out_old + fp32(s) each round once"""
    return np.abs(s) + np.abs(ref) + k * 2.0 ** -29 * S


def f32_in_order(terms):
    """the same sum accumulated in fp32 in list order (what the kernels must NOT do)"""
    acc = terms[0].astype(F32).copy()
    for t in terms[1:]:
        acc = (acc + t.astype(F32)).astype(F32)
    return acc


def f64_sum(terms):
    """(sum, sum of absolute values) in fp64"""
    s, a = np.zeros(terms[0].shape, F64), np.zeros(terms[0].shape, F64)
    for t in terms:
        s += t.astype(F64)
        a += np.abs(t.astype(F64))
    return s, a


# ====================================================================================================================
# data of the summing kernels: terms[k] fp32, all of one shape
# ====================================================================================================================
def cancelling(name, k, shape):
    """terms 0 .. k-2 Gaussian x 1e4, the last -fp32(their fp64 sum) + Gaussian x 1e-3.  k = 1: one Gaussian x 1e4 term (nothing cancels)"""
    g = rng(name)
    terms = [(g.standard_normal(shape) * 1e4).astype(F32) for _ in range(max(k - 1, 1))]
    if k > 1:
        s, _ = f64_sum(terms)
        terms.append((-s.astype(F32).astype(F64) + g.standard_normal(shape) * 1e-3).astype(F32))
    return terms


LATTICE_UNIT_EXP = (-6, 3, -11, 0)           # term k's unit: 2^(LATTICE_UNIT_EXP[k % 4]); the smallest, 2^-11, is the lattice unit


def lattice(name, k, shape):
    g = rng(name)
    return [(g.integers(-3, 4, shape) * 2.0 ** LATTICE_UNIT_EXP[i % 4]).astype(F32) for i in range(k)]


def lattice_span(terms):
    """max S / unit, unit the smallest unit of the terms"""
    unit = 2.0 ** min(LATTICE_UNIT_EXP[i % 4] for i in range(len(terms)))
    return float(f64_sum(terms)[1].max() / unit)


WIDE_A = 2.0 ** 26


def wide_lattice(name, k, shape):
    """k >= 3: +A m, small integers ..., -A m (m = 1 .. 3, A = 2^26, unit 1): exact in fp64, the result representable, fp32 partial sums are not"""
    assert k >= 3
    g = rng(name)
    m = g.integers(1, 4, shape).astype(F64)
    small = [g.integers(-3, 4, shape).astype(F32) for _ in range(k - 2)]
    small[0] = (2 * g.integers(0, 2, shape) + 1).astype(F32)                  # odd: A m + small[0] is never an fp32 number
    return [(WIDE_A * m).astype(F32)] + small + [(-WIDE_A * m).astype(F32)]


def gaussian(name, k, shape):
    """nothing cancels: the result needs all 24 bits, so the ONE rounding to fp32 is what the bar's first term meets (on the cancelling data the
    result is a short number and that rounding is exact)"""
    g = rng(name)
    return [g.standard_normal(shape).astype(F32) for _ in range(k)]


def make_terms(kind, name, k, shape):
    return {"cancel": cancelling, "lattice": lattice, "wide": wide_lattice, "gauss": gaussian}[kind](name, k, shape)


# ====================================================================================================================
# pooling
# ====================================================================================================================
def out_size(n):
    """ceil_mode: ceil((n - 3) / 2) + 1 (the last window starts inside the input for every n >= 1)"""
    return cdiv(n - 3, 2) + 1


def out_size_floor(n):
    return (n - 3) // 2 + 1


def _windows(a, Ho, Wo, absent):
    """a [N, H, W, C] -> for q = ky * 3 + kx the slab [N, Ho, Wo, C] of window element q and whether it lies inside the input"""
    N, H, W, C = a.shape
    p = np.full((N, 2 * Ho + 1, 2 * Wo + 1, C), absent, dtype=a.dtype)
    p[:, :H, :W] = a
    inside = np.zeros((2 * Ho + 1, 2 * Wo + 1), bool)
    inside[:H, :W] = True
    for q in range(9):
        ky, kx = divmod(q, 3)
        yield q, p[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2], inside[ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2][None, :, :, None]


def pool_fwd(x, rule="first"):
    """x [N, H, W, C] (any float type; selection only, so exact) -> (y [N, Ho, Wo, C], position bytes uint8).  rule "first": the kernel's and
    ATen's, `a > m || isnan(a)`; "last": `a >= m || isnan(a)`, the variant the CPU module shows to fail"""
    N, H, W, C = x.shape
    Ho, Wo = out_size(H), out_size(W)
    m = np.full((N, Ho, Wo, C), -np.inf, dtype=x.dtype)
    pos = np.zeros((N, Ho, Wo, C), np.uint8)
    with np.errstate(invalid="ignore"):
        for q, a, inside in _windows(x, Ho, Wo, 0):
            upd = inside & (((a > m) if rule == "first" else (a >= m)) | np.isnan(a))
            m = np.where(upd, a, m)
            pos = np.where(upd, np.uint8(q), pos)
    return m, pos


def pool_bwd(dy, pos, H, W):
    """dx[n, 2 oy + ky, 2 ox + kx, c] += dy[n, oy, ox, c] for the window's byte ky * 3 + kx, in fp64; with dy = |dy| it is S"""
    N, Ho, Wo, C = dy.shape
    p = np.zeros((N, 2 * Ho + 1, 2 * Wo + 1, C), F64)
    for q in range(9):
        ky, kx = divmod(q, 3)
        p[:, ky:ky + 2 * Ho:2, kx:kx + 2 * Wo:2] += np.where(pos == q, dy.astype(F64), 0.0)
    assert not p[:, H:].any() and not p[:, :, W:].any(), "a position byte points outside the input"
    return p[:, :H, :W]


def tie_stats(x, pos):
    """(windows, windows in which the maximum occurs more than once, windows whose first and last maximum differ) on NaN-free data"""
    last = pool_fwd(x, "last")[1]
    y = pool_fwd(x)[0]
    cnt = np.zeros(y.shape, int)
    for _, a, inside in _windows(x, y.shape[1], y.shape[2], 0):
        cnt += inside & (a == y)
    return y.size, int((cnt > 1).sum()), int((last != pos).sum())


PoolCase = namedtuple("PoolCase", "name N H W C kind")
POOL_SHAPES = ((1, 2, 2, 4), (1, 3, 3, 4), (2, 4, 7, 8), (1, 5, 6, 260), (3, 8, 9, 12), (1, 17, 23, 64))
POOL_BIG = (1, 1451, 1461, 4)          # 725 x 730 output quads > 2048 x 256, 1451 x 1461 input quads > 8192 x 256: a second grid-stride pass each
POOL_NAN = (1, 7, 7, 4)                # 3 x 3 windows; NaN placed by hand (pool_data)


def pool_cases():
    out = [PoolCase(f"{N}x{H}x{W}x{C}-{kind}", N, H, W, C, kind) for (N, H, W, C) in POOL_SHAPES for kind in ("int", "gauss")]
    out.append(PoolCase("%dx%dx%dx%d-int" % POOL_BIG, *POOL_BIG, "int"))
    out.append(PoolCase("2x4x7x8-neginf", 2, 4, 7, 8, "neginf"))
    out.append(PoolCase("%dx%dx%dx%d-nan" % POOL_NAN, *POOL_NAN, "nan"))
    return out


def pool_data(c):
    """(x, dy) fp32.  int: integers 0 .. 3 (ties), integer dy -3 .. 3.  neginf: sample 0's first window and all of channel 1 hold -inf.
    nan (channels 0 and 2; 1 and 3 stay finite): (1,1) NaN then (1,2) = 100 -- window (0,0) has ONE NaN followed by a larger finite value; (3,3) and
    (3,4) NaN -- window (1,1) has TWO (the byte is the last one's, 5), window (1,2) one, at its byte 3"""
    g = rng("pool-" + c.name)
    shape, oshape = (c.N, c.H, c.W, c.C), (c.N, out_size(c.H), out_size(c.W), c.C)
    if c.kind == "int":
        return g.integers(0, 4, shape).astype(F32), g.integers(-3, 4, oshape).astype(F32)
    x, dy = g.standard_normal(shape).astype(F32), g.standard_normal(oshape).astype(F32)
    if c.kind == "neginf":
        x[0, 0:3, 0:3, :] = -np.inf
        x[:, :, :, 1] = -np.inf
    if c.kind == "nan":
        for ch in (0, 2):
            x[0, 1, 1, ch], x[0, 1, 2, ch] = np.nan, 100.0
            x[0, 3, 3, ch] = x[0, 3, 4, ch] = np.nan
    return x, dy


def nan_count(x):
    """NaNs per window [N, Ho, Wo, C]"""
    Ho, Wo = out_size(x.shape[1]), out_size(x.shape[2])
    return sum((inside & np.isnan(a)).astype(int) for _, a, inside in _windows(x, Ho, Wo, 0))


# ====================================================================================================================
# sp_colsum
# ====================================================================================================================
CB, RL, MAX_G, COLSUM_SMALL_M = 64, 16, 256, 128


def pick_G(M, C):
    """the launcher's slab count: ~2048 blocks over the column blocks, at least 8 rows per thread, at most 256"""
    return max(1, min(cdiv(2048, cdiv(C, CB)), cdiv(M, RL * 8), MAX_G))


def colsum_path(M):
    return "one-launch" if M <= COLSUM_SMALL_M else "two-stage"


# M -> the G the issue intends (None: one launch, no slabs).  3072 and 4096 (G = 24, 32: the last sizes before the second stage's unrolled round
# of 32 slabs gains a remainder / a second round) are additions
COLSUM_M = {1: None, 3: None, 4: None, 5: None, 127: None, 128: None, 129: 2, 897: 8, 1024: 8, 1025: 9, 3072: 24, 3073: 25, 4096: 32, 4097: 33,
            32769: 256}
COLSUM_C = (4, 60, 64, 68, 260)
COLSUM_WIDE = (4224, 4096)             # cdiv(2048, 64 column blocks) = 32 caps G, not cdiv(M, 128) = 33
# (ld - C, beta, extra offset of x in words): ld and beta in full, the offset on two of the four
COLSUM_VARIANTS = ((0, 0, 0), (12, 1, 0), (0, 1, 4), (12, 0, 4))
ColsumCase = namedtuple("ColsumCase", "name M C G kind")


def colsum_cases():
    out = [ColsumCase(f"M{M}-C{C}-{kind}", M, C, G, kind) for (M, G), C in itertools.product(COLSUM_M.items(), COLSUM_C)
           for kind in ("cancel", "lattice")]
    out.append(ColsumCase("M%d-C%d-cancel" % COLSUM_WIDE, *COLSUM_WIDE, 32, "cancel"))
    out += [ColsumCase(f"M{M}-C68-{kind}", M, 68, COLSUM_M[M], kind) for M in (5, 128, 4097) for kind in ("wide", "gauss")]
    return out


COLSUM_UNIT_EXP = (-5, -4)            # lattice: row r's unit 2^COLSUM_UNIT_EXP[r % 2]: S / 2^-5 <= 6 M, far below 2^24 at M = 32769


def colsum_data(c):
    """(x [M, C] fp32, out_old [C] fp32: what out holds before a beta = 1 launch); the plan of make_terms with the rows as terms, drawn at once"""
    g, M, C = rng("colsum-" + c.name), c.M, c.C
    if c.kind == "cancel":
        x = (g.standard_normal((M, C)) * 1e4).astype(F32)
        if M > 1:
            x[-1] = (-x[:-1].astype(F64).sum(0).astype(F32).astype(F64) + g.standard_normal(C) * 1e-3).astype(F32)
        old = (g.standard_normal(C) * 1e-3).astype(F32)
    elif c.kind == "lattice":
        x = (g.integers(-3, 4, (M, C)) * np.where(np.arange(M) % 2, 2.0 ** COLSUM_UNIT_EXP[1], 2.0 ** COLSUM_UNIT_EXP[0])[:, None]).astype(F32)
        old = (g.integers(-3, 4, C) * 2.0 ** COLSUM_UNIT_EXP[0]).astype(F32)
    elif c.kind == "gauss":
        x, old = g.standard_normal((M, C)).astype(F32), g.standard_normal(C).astype(F32)
    else:
        x = np.stack(wide_lattice("colsum-" + c.name, M, (C,)))
        old = g.integers(-3, 4, C).astype(F32)
    return x, old


def colsum_ref(x, old, beta):
    """(ref, S', s, S): ref = beta old + s in fp64, S' the bar's argument (rounded once / twice)"""
    s, S = f64_sum(list(x))
    if not beta:
        return s, rounded_once(s, S, x.shape[0]), s, S
    ref = s + old.astype(F64)
    return ref, rounded_twice(s, ref, S + np.abs(old.astype(F64)), x.shape[0]), s, S + np.abs(old.astype(F64))


# ====================================================================================================================
# sp_sum_n / sp_sum_n_mixed
# ====================================================================================================================
SUM_COUNTS = (1, 2, 3, 31, 32)
SUM_N = (4, 8, 1020, 1024, 1028)
SUM_BIG = (2, 4 * (EW_CAP * EW_BLOCK + 3))            # (count, n): a second grid-stride pass of three quads
MIXED_N = (16, 32, 16 * 257)
MIXED_BIG = (2, 16 * (EW_CAP * EW_BLOCK + 1))
MIXED_LISTS = ("fp32", "split", "alternating")
SumCase = namedtuple("SumCase", "name count n kind")
MixedCase = namedtuple("MixedCase", "name count n forms kind")


def sum_cases():
    out = [SumCase(f"k{k}-n{n}-{kind}", k, n, kind) for k, n in itertools.product(SUM_COUNTS, SUM_N) for kind in ("cancel", "lattice")]
    out.append(SumCase("k%d-n%d-cancel" % SUM_BIG, *SUM_BIG, "cancel"))
    out += [SumCase(f"k{k}-n1028-wide", k, 1028, "wide") for k in (3, 32)]
    out += [SumCase(f"k{k}-n1028-gauss", k, 1028, "gauss") for k in SUM_COUNTS]
    return out


def mixed_cases():
    out = [MixedCase(f"k{k}-n{n}-{forms}-{kind}", k, n, forms, kind) for k, n, forms in itertools.product(SUM_COUNTS, MIXED_N, MIXED_LISTS)
           for kind in ("cancel", "lattice")]
    out.append(MixedCase("k%d-n%d-alternating-cancel" % MIXED_BIG, *MIXED_BIG, "alternating", "cancel"))
    out += [MixedCase(f"k{k}-n4112-fp32-wide", k, 16 * 257, "fp32", "wide") for k in (3, 32)]
    return out


def is_split(forms, k):
    return forms == "split" or (forms == "alternating" and k % 2 == 0)


SPLIT_EXP = tuple((5 * i) % 21 - 8 for i in range(21))             # 2^-8 .. 2^12, each once: term k's scale is 2^SPLIT_EXP[k % 21]


def split_scale(k):
    return 2.0 ** SPLIT_EXP[k % 21]


def split_planes(x, s):
    """hi = fp16(x s), lo = fp16(x s - hi) in the layout [group of 16][plane][16] -> uint16 [n / 16, 2, 16].  Built here, not by the project's
    splitter: x s and x s - hi are exact in fp64 (s a power of two, hi 11 bits of a 24-bit x)"""
    v = x.astype(F64) * s
    hi = v.astype(F16)
    lo = (v - hi.astype(F64)).astype(F16)
    assert np.isfinite(hi.astype(F64)).all(), "x s overflows fp16"
    return np.stack([hi.reshape(-1, 16), lo.reshape(-1, 16)], axis=1).view(np.uint16)


def decode_planes(planes, s):
    """the fp64 value the kernel reads from a split term: (hi + lo) / s"""
    p = planes.view(F16).astype(F64)
    return ((p[:, 0] + p[:, 1]) / s).reshape(-1)


def planes_sum_exact_in_f32(planes):
    """fp16 + fp16 is one fp32 number for every element"""
    p = planes.view(F16)
    return bool(((p[:, 0].astype(F32) + p[:, 1].astype(F32)).astype(F64) == p[:, 0].astype(F64) + p[:, 1].astype(F64)).all())


class Mixed:
    """the operands of one sp_sum_n_mixed launch (c: anything with name, count, n, forms, kind): term k is fp32 (f32[k]) or split (planes[k],
    scale[k]; f32[k] None -- its tensor is absent); value[k], fp64: what the kernel adds.  Gaussian terms have amplitude 5e3 / s, so that x s fits
    fp16 at every scale 2^-8 .. 2^12 (5e3 x 6 sigma < 65504); the last one cancels the others at a scale of its own (the largest with
    |x s| < 2^15, inside 2^-8 .. 2^12) and leaves 1e-7 of the largest sum, the ratio of sp_sum_n's 1e-3 to 1e4.  The scales are 2^SPLIT_EXP[k % 21]:
    all 21 of 2^-8 .. 2^12 before one repeats.  Lattice terms use 2^0 .. 2^4 (their units reach down to 2^-11, and x s must stay a normal fp16)"""
    def __init__(self, c):
        self.c = c
        g = rng("mixed-" + c.name)
        n, k = c.n, c.count
        self.f32, self.planes, self.scale, self.value = [None] * k, [None] * k, [None] * k, [None] * k
        raw = make_terms(c.kind, "mixed-" + c.name, k, (n,)) if c.kind != "cancel" else None
        for i in range(k):
            split = is_split(c.forms, i)
            s = split_scale(i) if split else 1.0
            if c.kind == "cancel":
                if i < k - 1 or k == 1:
                    x = (g.standard_normal(n) * (5e3 / s)).astype(F32)
                else:
                    tot = np.sum(self.value[:-1], axis=0)
                    x = (-tot.astype(F32).astype(F64) + g.standard_normal(n) * 1e-7 * np.abs(tot).max()).astype(F32)
                    if split:
                        s = 2.0 ** min(12, max(-8, 14 - int(np.ceil(np.log2(np.abs(x).max())))))
            else:
                x = raw[i]
                if split:                                 # lattice: integers x 2^e; x s stays an integer x power of two inside fp16's range
                    s = 2.0 ** (SPLIT_EXP[i % 21] % 5)
            if split:
                self.planes[i], self.scale[i] = split_planes(x, s), s
                self.value[i] = decode_planes(self.planes[i], s)
            else:
                self.f32[i], self.value[i] = x, x.astype(F64)

    def ref(self, live=None):
        """(ref, S) over the terms, live [count][n] bool: which words count (None: all)"""
        vals = [v if live is None else np.where(live[i], v, 0.0) for i, v in enumerate(self.value)]
        return f64_sum(vals)


# ---- row sparsity ----------------------------------------------------------------------------------------------------
STEPS = {"with-free": lambda k: [(7 * i + 2) % k - 1 for i in range(k)],           # unsorted, holds -1: a term no step owns, never skipped
         "all-owned": lambda k: [(7 * i + 2) % k for i in range(k)]}               # unsorted, 0 .. k-1: a sample with row_last -1 has no live term


def row_lasts(ns, k):
    """row_last holds -1, a middle step and a value above every step (one sample: one launch each)"""
    mid, above = k // 2, k + 3
    return {1: ([-1], [mid], [above]), 3: ([-1, mid, above],), 5: ([above, -1, mid, 0, mid + 1],)}[ns]


RowsCase = namedtuple("RowsCase", "name count n nsamples per steps row_last forms kind")
ROWS_PER = (4, 260)                    # elements per sample, sp_sum_n
MIXED_ROWS_PER = (16, 272)             # ... sp_sum_n_mixed (whole groups of 16)


def rows_cases(pers=ROWS_PER, lists=("fp32",)):
    out = []
    for k, ns, per, st, forms in itertools.product((5, 32), (1, 3, 5), pers, STEPS, lists):
        for rl in row_lasts(ns, k):
            for kind in ("cancel", "lattice"):
                name = f"k{k}-ns{ns}-per{per}-{st}-last{'.'.join(map(str, rl))}-{forms}-{kind}"
                out.append(RowsCase(name, k, ns * per, ns, per, tuple(STEPS[st](k)), tuple(rl), forms, kind))
    return out


def live_mask(c):
    """[count][n] bool: term k is read for sample b iff steps[k] <= row_last[b] (a step of -1 is never above a row_last >= -1)"""
    live = np.array(c.steps)[:, None] <= np.array(c.row_last)[None, :]
    return np.repeat(live, c.per, axis=1)


def rows_data(c):
    """terms fp32 [count][n]; they cancel where every term is live (a row_last above every step); dead words are finite here, the tests overwrite
    them with NaN"""
    return make_terms(c.kind, "rows-" + c.name, c.count, (c.n,))


# ====================================================================================================================
# layout, add, ReLU gradient
# ====================================================================================================================
NHWC_CASES = ((1, 1, 1, 1, 1), (1, 3, 5, 7, 4), (2, 3, 4, 4, 3), (1, 5, 3, 3, 8), (1, 3, 2, 2, 64), (1, 3, 363, 363, 4))          # N, C, H, W, Cp
PAD_CASES = ((1, 1, 1), (5, 3, 4), (7, 4, 3), (3, 5, 5), (1, 64, 1), (0, 3, 4), (131073, 3, 4))                                  # rows, Cin, Cout
ADD_N = (1, 3, 4, 5, 1023, 1024, 1027, 4 * EW_CAP * EW_BLOCK + 7)
RELU_N = (1, 255, 256, 257, EW_CAP * EW_BLOCK + 1)


def nhwc_ref(x, Cp):
    """x [N, C, H, W] -> [N, H, W, Cp], the extra channels +0.0"""
    N, C, H, W = x.shape
    y = np.zeros((N, H, W, Cp), x.dtype)
    y[..., :C] = x.transpose(0, 2, 3, 1)
    return y


def pad_ref(x, Cout):
    rows, Cin = x.shape
    y = np.zeros((rows, Cout), x.dtype)
    y[:, :min(Cin, Cout)] = x[:, :min(Cin, Cout)]
    return y


def relu_data(n):
    """(dy, y): y cycles through +0, -0, negatives, positives and NaN; dy holds inf and NaN under y <= 0 and under y = NaN"""
    g = rng(f"relu-{n}")
    y, dy = g.standard_normal(n).astype(F32), g.standard_normal(n).astype(F32)
    special = np.array([0.0, -0.0, -1.5, np.nan, 2.0, -np.inf, np.inf], F32)
    idx = np.arange(n)
    y[idx % 3 == 0] = special[(idx[idx % 3 == 0] // 3) % 7]
    dy[idx % 5 == 0] = np.array([np.inf, np.nan, -np.inf], F32)[(idx[idx % 5 == 0] // 5) % 3]
    return dy, y


def relu_ref(dy, y):
    """where(y > 0, dy, +0): no product, so dy = inf or NaN under y <= 0 (or y = NaN) gives +0"""
    with np.errstate(invalid="ignore"):
        return np.where(y > 0, dy, F32(0.0))
