"""Plain fp64 restatement, index by index, of what include/scanpaths_amd.h states for the entry points of csrc/head_direct.hip -- the reference
side of tests/test_head_direct_ref_cpu.py and tests/test_head_direct_gpu.py.  Nothing here touches a GPU.

Every function returns (ref, S): S is the same contraction over absolute values, the scale of the element-wise bar
|got - ref| <= c 2^-24 S + 2^-149 (parity.bar) with c the kernel's longest chain of dependent fp32 roundings plus one (gemm_ref's convention:
(1 + u)^c - 1 <= (c + 1) u, the one also covers the fp64 reference's own error).  The chains are read off the kernels and written next to each
chain_* function; nothing here was tuned on results.  tests/test_head_direct_ref_cpu.py holds the restatement to torch's fp64 conv2d and autograd
on the literal two-conv formulation.  `drop=True` leaves one term out of every sum (the teeth of the bars).

Layouts: G [nheads][HC][5][5][C] (rows 2 .. 50 of a head: the 49 duration taps), cb [nheads][HC], W11 [nheads][ncls][121][C], cbsum [nheads][ncls],
T [B][P][ldt] (column (src 2 + o) 25 + tap), Z2 [B][P][nsel 2], hmap [B][nsel], h / dh [B][P][C], Dpre / dDpre / live [nsel][B][S]."""
from collections import namedtuple

import numpy as np
import torch

from parity import cdiv, seed_of

MAXSITE, NV = 32, 121


# ====================================================================================================================
# sites and border classes
# ====================================================================================================================
def sites(n):
    return 0 if n < 3 else (n - 3) // 5 + 1


Axis = namedtuple("Axis", "len n masks cls")          # masks: one tuple of 7 booleans per class, in order of first appearance; cls: site -> class


def axis(n):
    """None for an illegal side (no site, or more than 32)"""
    ns = sites(n)
    if ns < 1 or ns > MAXSITE:
        return None
    masks, cls = [], []
    for s in range(ns):
        m = tuple(0 <= 5 * s - 2 + k < n for k in range(7))
        if m not in masks:
            masks.append(m)
        cls.append(masks.index(m))
    return Axis(n, ns, masks, cls)


def num_classes(Hm, Wm):
    ay, ax = axis(Hm), axis(Wm)
    return -1 if ay is None or ax is None else len(ay.masks) * len(ax.masks)


class Geo:
    """sites, classes and windows of an Hm x Wm map"""
    def __init__(self, Hm, Wm):
        self.Hm, self.Wm, self.P = Hm, Wm, Hm * Wm
        self.ay, self.ax = axis(Hm), axis(Wm)
        self.S, self.ncls = self.ay.n * self.ax.n, len(self.ay.masks) * len(self.ax.masks)
        self.cls = [self.ay.cls[s // self.ax.n] * len(self.ax.masks) + self.ax.cls[s % self.ax.n] for s in range(self.S)]
        # win[s][v]: the pixel under tap v of site s's 11 x 11 window (origin 5 s - 4), or P (an extra all-zero pixel) outside the map
        self.win = np.full((self.S, NV), self.P, dtype=np.int64)
        for s in range(self.S):
            sy, sx = divmod(s, self.ax.n)
            for v in range(NV):
                y, x = 5 * sy - 4 + v // 11, 5 * sx - 4 + v % 11
                if 0 <= y < Hm and 0 <= x < Wm:
                    self.win[s, v] = y * Wm + x

    def mask(self, c):
        return self.ay.masks[c // len(self.ax.masks)], self.ax.masks[c % len(self.ax.masks)]

    def max_taps(self):
        """most in-map taps of a window"""
        return int((self.win < self.P).sum(1).max())

    def max_class_sites(self):
        return max(self.cls.count(c) for c in range(self.ncls))


def _both(f, *tensors, **kw):
    """(f(tensors), f(|tensors|)): ref and S of a contraction that is linear in each tensor"""
    return f(*tensors, **kw), f(*(None if t is None else t.abs() for t in tensors), **{**kw, "drop": False})


# ====================================================================================================================
# compose11
# ====================================================================================================================
def _compose11_fwd(G, cb, geo, drop=False):
    nh, C = G.shape[0], G.shape[-1]
    W11 = torch.zeros(nh, geo.ncls, 11, 11, C, dtype=torch.float64)
    cbsum = torch.zeros(nh, geo.ncls, dtype=torch.float64)
    for c in range(geo.ncls):
        my, mx = geo.mask(c)
        taps = [(ky, kx) for ky in range(7) for kx in range(7) if my[ky] and mx[kx]]
        for vy in range(11):
            for vx in range(11):
                terms = [(ky, kx) for ky, kx in taps if 0 <= vy - ky <= 4 and 0 <= vx - kx <= 4]
                for ky, kx in terms[:-1] if drop else terms:
                    W11[:, c, vy, vx] += G[:, 2 + ky * 7 + kx, vy - ky, vx - kx]
        for ky, kx in taps[:-1] if drop else taps:
            cbsum[:, c] += cb[:, 2 + ky * 7 + kx]
    return W11.reshape(nh, geo.ncls, NV, C), cbsum


def compose11_fwd(G, cb, geo, drop=False):
    """W11[hd][cls][v] = sum over the 7 x 7 taps k inside the class's masks with u = v - k in the 5 x 5 filter of G[hd][2 + k][u];
    cbsum[hd][cls] = sum over the same taps of cb[hd][2 + k].  -> ((W11, cbsum), (S_W11, S_cbsum))"""
    return _both(_compose11_fwd, G.double(), cb.double(), geo=geo, drop=drop)


def _compose11_bwd(dW11, dcbsum, geo, HC, drop=False):
    nh, C = dW11.shape[0], dW11.shape[-1]
    dG = torch.zeros(nh, HC, 5, 5, C, dtype=torch.float64)
    dcb = torch.zeros(nh, HC, dtype=torch.float64)
    d = dW11.reshape(nh, geo.ncls, 11, 11, C)
    for ky in range(7):
        for kx in range(7):
            inside = [c for c in range(geo.ncls) if geo.mask(c)[0][ky] and geo.mask(c)[1][kx]]
            for c in inside[:-1] if drop else inside:
                dG[:, 2 + ky * 7 + kx] += d[:, c, ky:ky + 5, kx:kx + 5]
                dcb[:, 2 + ky * 7 + kx] += dcbsum[:, c]
    return dG, dcb


def compose11_bwd(dW11, dcbsum, geo, HC, drop=False):
    """the adjoint: dG[hd][2 + k][u] = sum over the classes whose masks hold tap k of dW11[hd][cls][k + u]; dcb alike; every other row of dG / dcb
    is zero.  -> ((dG, dcb), (S, S))"""
    return _both(_compose11_bwd, dW11.double(), dcbsum.double(), geo=geo, HC=HC, drop=drop)


# ====================================================================================================================
# sal_gather
# ====================================================================================================================
def _sal_gather_fwd(T, hmap, Hm, Wm, nsel, drop=False):
    B, ldt = T.shape[0], T.shape[-1]
    Tm, Z2 = T.reshape(B, Hm, Wm, ldt), torch.zeros(B, Hm, Wm, nsel * 2, dtype=torch.float64)
    py, px = torch.arange(Hm).reshape(-1, 1), torch.arange(Wm).reshape(1, -1)
    last = (Hm + 1 - py).clamp(max=4) * 5 + (Wm + 1 - px).clamp(max=4)              # a pixel's last tap inside the map
    for b in range(B):
        for j in range(nsel * 2):
            col0 = (int(hmap[b, j >> 1]) * 2 + (j & 1)) * 25
            for uy in range(5):
                y0, y1 = max(0, 2 - uy), min(Hm, Hm + 2 - uy)                       # the pixels p with q = p + u - 2 inside the map
                for ux in range(5):
                    x0, x1 = max(0, 2 - ux), min(Wm, Wm + 2 - ux)
                    if y0 >= y1 or x0 >= x1:
                        continue
                    t = Tm[b, y0 + uy - 2:y1 + uy - 2, x0 + ux - 2:x1 + ux - 2, col0 + uy * 5 + ux]
                    if drop:
                        t = t * (last[y0:y1, x0:x1] != uy * 5 + ux)
                    Z2[b, y0:y1, x0:x1, j] += t
    return Z2.reshape(B, Hm * Wm, nsel * 2)


def sal_gather_fwd(T, hmap, Hm, Wm, nsel, drop=False):
    """Z2[b][p][2 s + o] = sum over the 5 x 5 taps u with q = p + u - 2 inside the map of T[b][q][(hmap[b][s] 2 + o) 25 + u]"""
    return _both(_sal_gather_fwd, T.double(), hmap=hmap, Hm=Hm, Wm=Wm, nsel=nsel, drop=drop)


def _sal_gather_bwd(dZ2, hmap, Hm, Wm, nsel, nsrc, ldt, dead=(), drop=False):
    B = dZ2.shape[0]
    dZ, dT = dZ2.reshape(B, Hm, Wm, nsel * 2), torch.zeros(B, Hm, Wm, ldt, dtype=torch.float64)
    for b in range(B):
        if b in dead:
            continue
        for col in range(nsrc * 50):
            src, o, uy, ux = col // 50, (col % 50) // 25, (col % 25) // 5, col % 5
            y0, y1, x0, x1 = max(0, uy - 2), min(Hm, Hm + uy - 2), max(0, ux - 2), min(Wm, Wm + ux - 2)      # the q with p = q - (u - 2) inside the map
            if y0 >= y1 or x0 >= x1:
                continue
            slots = [s for s in range(nsel) if int(hmap[b, s]) == src]
            for s in slots[:-1] if drop else slots:
                dT[b, y0:y1, x0:x1, col] += dZ[b, y0 - uy + 2:y1 - uy + 2, x0 - ux + 2:x1 - ux + 2, s * 2 + o]
    return dT.reshape(B, Hm * Wm, ldt)


def sal_gather_bwd(dZ2, hmap, Hm, Wm, nsel, nsrc, ldt, dead=(), drop=False):
    """the adjoint: dT[b][q][(src 2 + o) 25 + u] = sum over the slots s with hmap[b][s] == src of dZ2[b][q - (u - 2)][2 s + o] (inside the map);
    columns >= 50 nsrc and the rows of dead samples are zeros (their dZ2, NaN in the tests, is not read: zeroed here first)"""
    d = dZ2.double().clone()
    d[list(dead)] = 0
    return _both(_sal_gather_bwd, d, hmap=hmap, Hm=Hm, Wm=Wm, nsel=nsel, nsrc=nsrc, ldt=ldt, dead=dead, drop=drop)


# ====================================================================================================================
# duration sites
# ====================================================================================================================
def dead_pairs(B, nsel, live=None, row_last=None, row_step=0, rowB=None):
    """on[i][b]: False where (row b, slot i) carries an exactly-zero gradient: live[i][b] == 0, or row_last[b % rowB] < row_step + b // rowB"""
    on = torch.ones(nsel, B, dtype=torch.bool)
    if live is not None:
        on &= torch.as_tensor(live).reshape(nsel, B) != 0
    if row_last is not None:
        rowB = B if rowB is None else rowB
        for b in range(B):
            if int(row_last[b % rowB]) < row_step + b // rowB:
                on[:, b] = False
    return on


def _windows(h, geo):
    """Hwin[b][s][v][c] = h[b][win(s, v)][c], zero outside the map"""
    B, P, C = h.shape
    hp = torch.cat([h, torch.zeros(B, 1, C, dtype=h.dtype)], 1)
    return hp[:, torch.from_numpy(geo.win)]


def _drt_fwd(h, W11, cbsum, hmap, geo, nsel, drop=False):
    B = h.shape[0]
    Hw = _windows(h, geo)                                                          # [B, S, 121, C]
    if drop:                                                                       # the last in-map tap of every window
        last = [int(np.nonzero(geo.win[s] < geo.P)[0][-1]) for s in range(geo.S)]
        Hw[:, torch.arange(geo.S), torch.tensor(last)] = 0
    D = torch.zeros(nsel, B, geo.S, dtype=torch.float64)
    for i in range(nsel):
        for b in range(B):
            k = int(hmap[b, i])
            D[i, b] = (W11[k, geo.cls] * Hw[b]).sum((1, 2)) + cbsum[k, geo.cls]
    return D


def drt_fwd(h, W11, cbsum, hmap, geo, nsel, drop=False):
    """Dpre[i][b][s] = cbsum[src][cls(s)] + sum over the window taps v inside the map and the channels of W11[src][cls(s)][v][c] h[b][win(s, v)][c],
    src = hmap[b][i]"""
    return _both(_drt_fwd, h.double(), W11.double(), cbsum.double(), hmap=hmap, geo=geo, nsel=nsel, drop=drop)


def _drt_bwd_data(dD, W11, dh0, hmap, geo, nsel, on, drop=False):
    B, C = dD.shape[1], W11.shape[-1]
    out = torch.zeros(B, geo.P + 1, C, dtype=torch.float64)
    idx = torch.from_numpy(geo.win).reshape(-1)
    last_site = {}                                                                 # pixel -> its last covering site
    for s in range(geo.S):
        for q in geo.win[s][geo.win[s] < geo.P]:
            last_site[int(q)] = s
    keep = torch.tensor([[not (geo.win[s, v] < geo.P and last_site[int(geo.win[s, v])] == s) for v in range(NV)] for s in range(geo.S)])
    for i in range(nsel):
        for b in range(B):
            if not on[i, b]:
                continue
            t = dD[i, b].reshape(geo.S, 1, 1) * W11[int(hmap[b, i]), geo.cls]        # [S, 121, C]
            if drop and i == nsel - 1:                                             # every pixel loses its last covering site in the last slot
                t = t * keep[:, :, None]
            out[b].index_add_(0, idx, t.reshape(-1, C))
    out = out[:, :geo.P]
    return out if dh0 is None else out + dh0


def drt_bwd_data(dD, W11, hmap, geo, nsel, dh0=None, on=None, drop=False):
    """dh[b][q][c] = (dh0[b][q][c] under accumulate) + sum over the slots i and the sites s whose window covers q of
    dDpre[i][b][s] W11[hmap[b][i]][cls(s)][v(s, q)][c]; the (row, slot) pairs with on == False contribute nothing"""
    on = torch.ones(nsel, dD.shape[1], dtype=torch.bool) if on is None else on
    return _both(_drt_bwd_data, dD.double(), W11.double(), None if dh0 is None else dh0.double(), hmap=hmap, geo=geo, nsel=nsel, on=on, drop=drop)


def _drt_bwd_weight(dD, h, hmap, geo, nsel, nheads, on, drop=None):
    B, C = h.shape[0], h.shape[-1]
    Hw = _windows(h, geo)
    dW = torch.zeros(nheads, geo.ncls, NV, C, dtype=torch.float64)
    dcs = torch.zeros(nheads, geo.ncls, dtype=torch.float64)
    onehot = torch.zeros(geo.S, geo.ncls, dtype=torch.float64)
    onehot[torch.arange(geo.S), torch.tensor(geo.cls)] = 1
    pairs = [(b, i) for b in range(B) for i in range(nsel)]
    for b, i in pairs:
        k = int(hmap[b, i])
        g = dD[i, b].clone()
        if drop == "slab" and (b, i) == [p for p in pairs if int(hmap[p]) == k][-1]:
            continue
        if drop == "site":
            g[geo.S - 1] = 0
        dcs[k] += g @ onehot
        if on[i, b]:
            dW[k] += torch.einsum("s,svc,sk->kvc", g, Hw[b], onehot)
    return dW, dcs


def drt_bwd_weight(dD, h, hmap, geo, nsel, nheads, on=None, drop=None):
    """dW11[k][cls][v][c] = sum over the pairs (b, i) with hmap[b][i] == k and on, over the sites s of the class, of dDpre[i][b][s] h[b][win(s, v)][c]
    (zero outside the map); dcbsum[k][cls] = sum over the same pairs (flags not applied: a dead pair's dDpre is zero by contract) and sites of
    dDpre[i][b][s].  drop: "slab" (the last pair of every head) or "site" (the last site).  -> ((dW11, dcbsum), (S, S))"""
    on = torch.ones(nsel, h.shape[0], dtype=torch.bool) if on is None else on
    f = lambda a, b_, drop: _drt_bwd_weight(a, b_, hmap, geo, nsel, nheads, on, drop)
    return f(dD.double(), h.double(), drop), f(dD.double().abs(), h.double().abs(), None)


# ====================================================================================================================
# chains of dependent roundings (each plus one, the convention of gemm_ref.py)
# ====================================================================================================================
def chain_compose11_fwd():
    """compose11_fwd_kernel: `acc += G4[..]` over at most 49 taps from 0.f (cbsum: the same 49 adds)"""
    return 49 + 1


def chain_compose11_bwd(ncls):
    """compose11_bwd_kernel, dG: `acc += S4[..]` over at most ncls classes.  (dcb is an fp64 sum rounded once: chain_dcbsum)"""
    return ncls + 1


def chain_sal_gather_fwd():
    """sal_gather_fwd_kernel: `acc += t[..]` over at most 25 taps"""
    return 25 + 1


def chain_sal_gather_bwd(nsel):
    """sal_gather_bwd_kernel: `v += dZ2[..]` over at most nsel slots"""
    return nsel + 1


def chain_drt_fwd(geo, C):
    """drt_fwd_kernel: a thread runs ceil(cnt C4 / 256) drt_dot4 of four fmaf each into one accumulator (cnt: the window's in-map taps);
    wave_sum: 6 adds; block_sum_256's sh4[0] + sh4[1] + sh4[2] + sh4[3]: 3; + cbsum: 1"""
    return 4 * cdiv(geo.max_taps() * (C // 4), 256) + 6 + 3 + 1 + 1


def chain_drt_bwd_data(nsel, accumulate):
    """drt_bwd_data_kernel: `acc[j] += g * w`, a multiply and an add (the compiler may fuse them or not: two) per term, at most 3 x 3 covering
    sites x nsel slots; `r += O4[o]` under accumulate"""
    return 2 * 9 * nsel + int(bool(accumulate)) + 1


def chain_drt_bwd_weight(geo, hmap, nheads):
    """drt_bwd_weight_kernel: `acc += s_g[k] * a[u]`, two per compacted site, at most the sites of the largest class; drt_slab_reduce_kernel:
    `acc += S4[..]` over the (b, i) pairs of a head"""
    pairs = max(int((torch.as_tensor(hmap) == k).sum()) for k in range(nheads))
    return 2 * geo.max_class_sites() + pairs + 1


def chain_dcbsum():
    """drt_dcbsum_kernel's dcbsum and compose11_bwd_kernel's dcb: fp64 sums, rounded to fp32 once"""
    return 1 + 1


# ====================================================================================================================
# cases and data
# ====================================================================================================================
# side -> (sites, classes): the issue's table, and 23 (the short side of the 23 x 133 map it lists)
SIDES = {3: (1, 1), 7: (1, 1), 8: (2, 2), 13: (3, 3), 15: (3, 2), 23: (5, 3), 38: (8, 3), 40: (8, 2), 133: (27, 3), 162: (32, 2)}

Case = namedtuple("HeadCase", "name Hm Wm B C nsel nheads HC hmap")


def _c(Hm, Wm, B, C, nsel, nheads, hmap, HC=64):
    return Case(f"{Hm}x{Wm}-B{B}-C{C}-nsel{nsel}-heads{nheads}-HC{HC}-{hmap}", Hm, Wm, B, C, nsel, nheads, HC, hmap)


def cases():
    """pairwise by hand over maps x B x C x nsel x nheads x hmap kind.  hmap: `same` for all rows; `mixed` differs inside a group of four rows;
    `unused` leaves the last head without a row.  38x8 / 40x13 run the XCD site order (ay.n == 8) with B = 4 and 5; 23x133 has S = 135 sites
    (second compaction round of drt_bwd_weight_kernel); C = 516 is C / 4 = 129 > 128 threads and cnt C4 = 9 x 129, no multiple of 256"""
    return [_c(3, 3, 1, 4, 1, 1, "same"), _c(3, 3, 4, 516, 2, 2, "mixed"), _c(7, 8, 3, 12, 3, 3, "unused"), _c(7, 8, 9, 4, 9, 2, "same", HC=51),
            _c(13, 15, 5, 12, 2, 3, "mixed"), _c(13, 15, 4, 4, 1, 2, "unused"), _c(38, 8, 4, 12, 2, 2, "same"), _c(38, 8, 5, 4, 3, 3, "mixed"),
            _c(40, 13, 5, 12, 1, 1, "same"), _c(40, 13, 4, 4, 9, 3, "mixed"), _c(8, 40, 3, 12, 2, 2, "same"), _c(8, 40, 9, 4, 3, 3, "unused"),
            _c(23, 133, 1, 4, 2, 2, "same"), _c(23, 133, 5, 4, 1, 3, "mixed"), _c(3, 162, 3, 4, 3, 1, "same"), _c(162, 3, 4, 4, 2, 2, "unused"),
            _c(3, 3, 9, 12, 9, 3, "unused"), _c(13, 15, 9, 12, 3, 1, "same"), _c(38, 8, 1, 12, 1, 3, "unused"), _c(40, 13, 3, 12, 2, 2, "unused"),
            _c(8, 40, 1, 4, 9, 1, "same"), _c(7, 8, 5, 12, 1, 2, "mixed"), _c(3, 162, 5, 12, 2, 3, "mixed"), _c(162, 3, 1, 4, 3, 3, "same"),
            _c(23, 133, 4, 4, 3, 1, "same"), _c(3, 3, 3, 4, 2, 3, "mixed"), _c(13, 15, 1, 12, 9, 2, "unused"), _c(38, 8, 9, 4, 2, 1, "same"),
            _c(40, 13, 9, 12, 3, 2, "mixed"), _c(8, 40, 4, 12, 1, 3, "mixed")]


def make_hmap(c):
    b, i = np.meshgrid(np.arange(c.B), np.arange(c.nsel), indexing="ij")
    if c.hmap == "same":
        m = i % c.nheads
    elif c.hmap == "mixed":
        m = (b + i) % c.nheads
    else:
        m = (b + i) % (c.nheads - 1)
    return torch.from_numpy(m.astype(np.int32))


def data(kind, shape, seed, power=0):
    """gauss: N(0, 1); lattice: integers in -3 .. 3 times 2^power"""
    g = np.random.Generator(np.random.PCG64(seed))
    if kind == "gauss":
        return torch.from_numpy(g.standard_normal(shape).astype(np.float32))
    return torch.from_numpy((g.integers(-3, 4, shape) * 2.0 ** power).astype(np.float32))


class Problem:
    """the operands of every entry point for one case; the lattice kinds' units (the product of the operand units) ride along"""
    def __init__(self, c, kind):
        self.c, self.kind, self.geo = c, kind, Geo(c.Hm, c.Wm)
        geo, s = self.geo, seed_of("head" + kind + c.name)
        self.hmap = make_hmap(c)
        d = lambda shape, n, power: data(kind, shape, s + n, power)
        self.G, self.cb = d((c.nheads, c.HC, 5, 5, c.C), 1, -3), d((c.nheads, c.HC), 2, -4)
        self.h = d((c.B, geo.P, c.C), 3, -2)
        self.W11, self.cbsum = d((c.nheads, geo.ncls, NV, c.C), 4, -3), d((c.nheads, geo.ncls), 5, -6)
        self.dW11, self.dcbsum = d((c.nheads, geo.ncls, NV, c.C), 6, -1), d((c.nheads, geo.ncls), 7, -2)
        self.dD = d((c.nsel, c.B, geo.S), 8, -1)
        self.dh0 = d((c.B, geo.P, c.C), 9, -5)
        self.unit = {"compose_fwd": 2.0 ** -3, "compose_fwd_cb": 2.0 ** -4, "compose_bwd": 2.0 ** -1, "compose_bwd_cb": 2.0 ** -2,
                     "gather": 2.0 ** -2, "drt_fwd": 2.0 ** -6, "bwd_data": 2.0 ** -5, "bwd_weight": 2.0 ** -3, "dcbsum": 2.0 ** -1}

    def T(self, nsrc, ldt):
        return data(self.kind, (self.c.B, self.geo.P, ldt), seed_of("T" + self.c.name), -2)

    def dZ2(self):
        return data(self.kind, (self.c.B, self.geo.P, self.c.nsel * 2), seed_of("dZ2" + self.c.name), -2)
