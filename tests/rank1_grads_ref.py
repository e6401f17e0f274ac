"""Plain fp64 restatement of sp_rank1_grads_f16x2 (csrc/rank1_grads.hip) -- the reference side of tests/test_rank1_grads_ref_cpu.py and
tests/test_rank1_grads_gpu.py.  Nothing here touches a GPU.

    dsp[b][p][k] = sum_{n < N3} dpre[b][p][n] wc[b][n][k]            dwc[b][n][k] = sum_p dpre[b][p][n] spcol[b][p][k]

OPERANDS as the kernel reads them.  dpre: the planes of sp_split2_f16 (f16x2_ref.split2 with the scalar scale sy) in rows of ldy halves per plane,
fp16 NaN in the pad columns (f16x2_ref.pack).  wc^T: the planes of sp_split2_f16_rows, rows (b, k), one scale per row.  The taps (spcol) stay fp32;
the kernel splits them itself, per workgroup = per (sample, chunk of 160 pixels): tap_scale = 2^(127 + 14 - e) with e the biased exponent of the
chunk's largest |tap|, the scale's own biased exponent clamped to [1, 254] (tap_scale below), th = fp16(x s), tl = fp16(x s - th) (split_taps).

TWO CONTRACTIONS, both fp64, as in f16x2_ref.py:
    R_planes   exactly the three products each side takes (high x high, high x low, low x high), divided by the scales; for dwc per chunk, the
               chunks added in chunk order
    R_true     the same contraction on the fp32 operands
BARS.  Kernel against R_planes: parity.bar(S, chain) with S the contraction over f16x2_ref.hw_abs magnitudes and the chains below (the
conventions and the UNMEASURED assumption of f16x2_ref.py: PROD_UNITS per product of v_mfma_f32_16x16x32_f16).  R_planes against R_true:
f16x2_ref.rep_bound(.., 3), per chunk for dwc.  Nothing here was tuned on results.

LATTICE DATA (f16x2_ref.lattice).  dpre and every row of wc^T carry one 8192 per scale group, so their planes are h and l exactly.  The taps
carry one 8192 / 2^q per (sample, chunk): the kernel's scale puts that maximum at 2^14 -- TWICE f16x2_ref.scale_of's 2^13 -- so th = 2 h and
tl = 2 l, still exact.  Accumulator units: 4096 for dsp, 8192 for dwc (low x high = 1 x 8192)."""
import itertools
from collections import namedtuple

import numpy as np
import torch

import f16x2_ref as X
from parity import cdiv, seed_of

F32, F16 = np.float32, np.float16
PX, NT = 32, 5                     # R1_PX, R1_NT: pixels per LDS tile, tiles per workgroup
CHUNK = PX * NT                    # 160 pixels per workgroup


def tap_scale(amax):
    """the workgroup's tap scale: `se = min(254, max(1, 268 - e))`, e = bits 23..30 of max |tap| (0 for an all-zero chunk: 2^127)"""
    e = (int(np.array(amax, dtype=F32).view(np.uint32)) >> 23) & 0xFF
    return np.array(min(254, max(1, 268 - e)) << 23, dtype=np.uint32).view(F32)[()]


def chunk_scales(taps):
    """[B][chunks] fp32"""
    B, P, _ = taps.shape
    return np.array([[tap_scale(X._amax(taps[b, c * CHUNK:(c + 1) * CHUNK])) for c in range(cdiv(P, CHUNK))] for b in range(B)], dtype=F32)


def split_taps(taps, s):
    """(th, tl) fp16 [B][P][KP] for the chunk scales s [B][chunks]: `x = tap * tap_scale; h = fp16(x); l = fp16(x - (float)h)`"""
    per_pixel = np.repeat(s, CHUNK, axis=1)[:, :taps.shape[1], None]
    return X.split2(taps, per_pixel)


# ====================================================================================================================
# chains of dependent roundings, in units of 2^-24 (f16x2_ref._chain, PROD_UNITS)
# ====================================================================================================================
def chain_dsp(N3):
    """dacc[tile] is ONE accumulator over all N3 / 32 k-steps (it lives across the channel chunks), three v_mfma_f32_16x16x32_f16 per k-step;
    the store multiplies by 1 / sy and 1 / sw: 2"""
    return X._chain(X.PROD_UNITS * 32 * 3 * (N3 // 32) + 2)


def chain_dwc(P):
    """wacc is one accumulator over the workgroup's pixel tiles (at most NT = 5) of a channel chunk, three instructions per 32-pixel tile;
    rank1_reduce_kernel runs `s += slab * slab_inv` per chunk, then multiplies by 1 / sy: 1.  The issue counts one add per chunk; here the
    multiply by 1 / tap_scale is counted too (2 per chunk: the compiler may or may not fuse the pair, and 2^-127 times a small slab can round in
    the subnormal range) -- at most 3 units more in about 970"""
    return X._chain(X.PROD_UNITS * 32 * 3 * min(NT, P // PX) + 2 * cdiv(P, CHUNK) + 1)


# ====================================================================================================================
# cases
# ====================================================================================================================
Case = namedtuple("Rank1Case", "name KP P N3 ldy B dead kind")

KPS, PS, N3S, BS = (12, 20), (32, 128, 160, 192, 320, 352), (256, 512, 768), (1, 3)
LDYS = ("dense", "plus16", "four-thirds")
DEADS = ("none", "all", "mixed")
KINDS = ("gauss", "lattice", "rows", "spread", "zero-chunk", "tiny-chunk", "huge-chunk")
SPECIAL_CHUNK = 0                  # the chunk the last three kinds fill; every other chunk is Gaussian


def _ok(KP, P, N3, ldy, B, dead, kind):
    if ldy == "four-thirds" and (4 * N3) % 3 or ldy == "four-thirds" and (4 * N3 // 3) % 16:
        return False
    if dead == "mixed" and B == 1:
        return False
    if kind.endswith("-chunk") and P <= CHUNK:             # the special chunk stands beside an ordinary one
        return False
    return True


def _ldy(N3, ldy):
    return {"dense": N3, "plus16": N3 + 16, "four-thirds": 4 * N3 // 3}[ldy]


def pairwise_cases():
    """greedy all-pairs over the axes of the issue's table (deterministic: the first best candidate of the full product), except the pair
    (P, data kind), whose 42 combinations alone would exceed the budget: every P and every kind still meets every value of every other axis"""
    axes = (KPS, PS, N3S, LDYS, BS, DEADS, KINDS)
    full = [c for c in itertools.product(*axes) if _ok(*c)]
    pairs = lambda c: {(i, c[i], j, c[j]) for i in range(7) for j in range(i + 1, 7) if (i, j) != (1, 6)}
    need = set().union(*(pairs(c) for c in full))
    chosen = []
    while need:
        best = max(full, key=lambda c: len(pairs(c) & need))
        need -= pairs(best)
        chosen.append(best)
    return [Case(f"KP{c[0]}-P{c[1]}-N{c[2]}-ldy-{c[3]}-B{c[4]}-dead-{c[5]}-{c[6]}", c[0], c[1], c[2], _ldy(c[2], c[3]), c[4], c[5], c[6]) for c in chosen]


def cases():
    """the pairwise list plus the single-workgroup extremes: one tile in total (the first wait is vmcnt(0)), one full chunk, and whole launches
    whose only chunk clamps its scale / carries huge taps / is all zeros; and the largest shape on lattice and on Gaussian data (the greedy list
    puts both kinds on one or four tiles only)"""
    cs = pairwise_cases()
    cs += [Case("one-tile-KP20", 20, 32, 256, 256, 1, "none", "gauss"), Case("one-tile-KP12-lattice", 12, 32, 256, 272, 3, "mixed", "lattice"),
           Case("one-chunk-tiny-all", 20, 160, 256, 256, 1, "none", "tiny-all"), Case("one-tile-huge-all", 12, 32, 512, 528, 1, "none", "huge-all"),
           Case("one-chunk-zero-all", 20, 160, 512, 512, 3, "none", "zero-all"),
           Case("three-chunks-two-channel-chunks-lattice", 20, 352, 512, 528, 3, "mixed", "lattice"),
           Case("three-chunks-three-channel-chunks-gauss", 20, 352, 768, 1024, 1, "none", "gauss")]
    return cs


# ====================================================================================================================
# the problem
# ====================================================================================================================
def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


class Problem:
    def __init__(self, c):
        self.c = c
        s = seed_of("rank1" + c.name)
        B, P, N3, KP = c.B, c.P, c.N3, c.KP
        self.chunks = cdiv(P, CHUNK)
        lat = c.kind == "lattice"
        # ---- operands (fp32) ----
        if lat:
            dpre = X.lattice((B, P, N3), (), s)[0]
            wcT = X.lattice((B, KP, N3), (0, 1), s + 1)[0]
            taps = np.concatenate([X.lattice((B, min(CHUNK, P - ch * CHUNK), KP), (0,), s + 10 + ch)[0] for ch in range(self.chunks)], axis=1)
        else:
            dpre = X.gauss((B, P, N3), s)
            if c.kind == "rows":                                                   # rows of different magnitudes
                dpre = (dpre * np.exp(X.gauss((B, P, 1), s + 3))).astype(F32)
            wcT = (X.gauss((B, KP, N3), s + 1) * F32(0.2)).astype(F32)
            taps = X.gauss((B, P, KP), s + 2)
            sp = slice(SPECIAL_CHUNK * CHUNK, (SPECIAL_CHUNK + 1) * CHUNK)
            if c.kind == "spread":                                                 # magnitudes 2^-20 .. 1 inside every chunk
                e = np.random.Generator(np.random.PCG64(s + 4)).integers(-20, 1, (B, P, KP))
                taps = (taps * np.exp2(e)).astype(F32)
            elif c.kind == "zero-chunk":
                taps[:, sp] = 0
            elif c.kind == "tiny-chunk":
                taps[:, sp] *= F32(2.0 ** -120)
            elif c.kind == "huge-chunk":
                taps[:, sp] *= F32(2.0 ** 100)
            elif c.kind == "tiny-all":
                taps *= F32(2.0 ** -120)
            elif c.kind == "huge-all":
                taps *= F32(2.0 ** 100)
            elif c.kind == "zero-all":
                taps[:] = 0
        self.dpre, self.wcT, self.taps = dpre, wcT, taps
        # ---- what the kernel reads ----
        self.sy = X.scale_of(X._amax(dpre))
        y1, y2 = X.split2(dpre.reshape(B * P, N3), self.sy)
        self.Yp = X.pack(y1, y2, c.ldy)
        self.Wp, self.sw = X.split2_f16_rows(wcT.reshape(B * KP, N3))
        w1, w2 = X.split2(wcT.reshape(B * KP, N3), self.sw[:, None])
        self.st = chunk_scales(taps)                                               # [B][chunks]
        th, tl = split_taps(taps, self.st)
        self.Y1, self.Y2 = _t(y1).reshape(B, P, N3), _t(y2).reshape(B, P, N3)
        self.W1, self.W2 = _t(w1).reshape(B, KP, N3).transpose(1, 2), _t(w2).reshape(B, KP, N3).transpose(1, 2)        # [B, N3, KP]
        self.T1, self.T2 = _t(th), _t(tl)                                          # [B, P, KP]
        self.f_dsp = 1.0 / (float(self.sy) * _t(self.sw).reshape(B, 1, KP))
        self.f_dwc = 1.0 / (float(self.sy) * _t(self.st).reshape(B, self.chunks, 1, 1))          # per chunk
        self.chain_dsp, self.chain_dwc = chain_dsp(N3), chain_dwc(P)
        # dead samples (row_last[b] < row_step = 5; the live ones sit exactly at the step)
        self.dead = {"none": [], "all": list(range(B)), "mixed": [b for b in range(B) if b != 1]}[c.dead]
        self.row_last = None if c.dead == "none" else np.array([2 if b in self.dead else 5 for b in range(B)], dtype=np.int32)
        self.row_step = 5

    def planes_with_dead_rows_nan(self):
        """the dpre operand with every half of the dead samples' rows an fp16 NaN"""
        c = self.c
        buf = self.Yp.copy()
        rows = buf[:2 * c.B * c.P * c.ldy].reshape(c.B, c.P * c.ldy * 2)
        rows[self.dead] = X.F16_NAN
        return buf

    # ---- dsp ----
    @staticmethod
    def _three(A1, A2, B1, B2, mag=lambda v: v):
        return torch.matmul(mag(A1), mag(B1)) + torch.matmul(mag(A1), mag(B2)) + torch.matmul(mag(A2), mag(B1))

    def dsp_planes(self, drop_group=None):
        """(R_planes, S) [B, P, KP]; drop_group: a group of 16 channels left out of every product"""
        k = slice(None) if drop_group is None else [n for n in range(self.c.N3) if n // 16 != drop_group]
        Y1, Y2, W1, W2 = self.Y1[:, :, k], self.Y2[:, :, k], self.W1[:, k], self.W2[:, k]
        return self._three(Y1, Y2, W1, W2) * self.f_dsp, self._three(Y1, Y2, W1, W2, X.hw_abs) * self.f_dsp

    def dsp_true(self):
        return torch.matmul(_t(self.dpre), _t(self.wcT).transpose(1, 2))

    def dsp_rep(self):
        absA = _t(self.dpre).abs() * float(self.sy)
        absB = (_t(self.wcT).abs() * _t(self.sw).reshape(self.c.B, self.c.KP, 1)).transpose(1, 2)
        return X.rep_bound(absA, absB, 3) * self.f_dsp + 1e-13 * self.dsp_planes()[1] + 2.0 ** -149

    # ---- dwc ----
    def dwc_planes(self, drop_pixel=None):
        """(R_planes, S) [B, N3, KP]: per chunk, divided by the chunk's scale, chunks added in chunk order"""
        ref = torch.zeros(self.c.B, self.c.N3, self.c.KP, dtype=torch.float64)
        S = torch.zeros_like(ref)
        for ch in range(self.chunks):
            px = [p for p in range(ch * CHUNK, min(self.c.P, (ch + 1) * CHUNK)) if p != drop_pixel]
            A1, A2, T1, T2 = self.Y1[:, px].transpose(1, 2), self.Y2[:, px].transpose(1, 2), self.T1[:, px], self.T2[:, px]
            ref = ref + self._three(A1, A2, T1, T2) * self.f_dwc[:, ch]
            S = S + self._three(A1, A2, T1, T2, X.hw_abs) * self.f_dwc[:, ch]
        return ref, S

    def dwc_true(self):
        return torch.matmul(_t(self.dpre).transpose(1, 2), _t(self.taps))

    def dwc_rep(self):
        r = torch.zeros(self.c.B, self.c.N3, self.c.KP, dtype=torch.float64)
        for ch in range(self.chunks):
            px = slice(ch * CHUNK, min(self.c.P, (ch + 1) * CHUNK))
            absA = _t(self.dpre)[:, px].abs().transpose(1, 2) * float(self.sy)
            absB = _t(self.taps)[:, px].abs() * _t(self.st)[:, ch].reshape(-1, 1, 1)
            r = r + X.rep_bound(absA, absB, 3) * self.f_dwc[:, ch]
        return r + 1e-13 * self.dwc_planes()[1] + 2.0 ** -149

    # ---- lattice ----
    def exact_spans(self):
        """(dsp, dwc): largest S / unit of the raw accumulations.  dsp: products are multiples of 4096 (1 x 4096), the scales are powers of
        two.  dwc: multiples of 8192 (1 x 8192, 4096 x 2) inside a chunk; across chunks the reducer's sum has the unit of its finest chunk"""
        dsp = float((self.dsp_planes()[1] / self.f_dsp).max()) / 4096.0
        unit = 8192.0 * self.f_dwc.min(dim=1).values                              # [B, 1, 1]
        return dsp, float((self.dwc_planes()[1] / unit).max())

    def teeth_pixel(self):
        """a pixel whose removal the bar must notice: the last pixel (never in the special chunk) -- but under huge-chunk the special chunk's
        last pixel: its 2^100 taps set S, beside them an ordinary pixel is below every bar"""
        return CHUNK - 1 if self.c.kind == "huge-chunk" else self.c.P - 1


# refusals: (name, KP, P, N3, ldy, B, byte offsets of planes / wc planes / workspace, applies)
Refusal = namedtuple("Rank1Refusal", "name KP P N3 ldy B offY offW offWs null rc applies")


def _rf(name, KP=20, P=160, N3=256, ldy=256, B=1, offY=0, offW=0, offWs=0, null=None, rc=-1, applies=0):
    return Refusal(name, KP, P, N3, ldy, B, offY, offW, offWs, null, rc, applies)


POINTERS = ("dpre_planes", "dpre_scale", "wcT_planes", "wcT_row_scale", "spcol", "dsp", "dwc", "workspace")


def refusals():
    return ([_rf(f"{n}-null", null=n, rc=-2, applies=1) for n in POINTERS]
            + [_rf("KP16", KP=16), _rf("P-not-32", P=168), _rf("P0", P=0), _rf("N3-128", N3=128, ldy=128), _rf("N3-not-256", N3=384, ldy=384),
               _rf("ldy-below-N3", ldy=240), _rf("ldy-not-16", ldy=264), _rf("B0", B=0), _rf("B65536", B=65536),
               _rf("planes+8B", offY=8, applies=1), _rf("wc-planes+8B", offW=8, applies=1), _rf("workspace+8B", offWs=8, applies=1)])
