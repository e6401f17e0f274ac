"""The yardstick of csrc/scankde.hip: a plain-loop float64 restatement of the definitions, one operation per line and
every sum in index order, and a vectorised `quick` form of the same definitions for inputs the plain loops are too slow for.  The plain
loops check the quick form (tests/test_scanpath_kde_cpu.py); the device is checked against either.

Frame (h, w), map (Hm, Wm), P = Hm * Wm.  The cell of a fixation: col = floor(x * Wm / w), row = floor(y * Hm / h), clamped to the last
cell; a fixation outside the frame or with a non-finite coordinate is dropped.  Cell centres cx(col) = (col + 0.5) * w / Wm, cy(row) =
(row + 0.5) * h / Hm.  The cell kernel of a source (x, y) at bandwidth b: wx(col) = exp(ax(col) - max ax) / sum_col exp(ax(col) - max ax)
with ax(col) = -(cx(col) - x)^2 / (2 b^2), wy(row) likewise, k(c) = wy(row(c)) * wx(col(c)).  Only the first min(n, max_length)
fixations of a scanpath count.  The leave-out score of a query i with cell c: q = (sum_{j in A_i} k_j(c)) / M, M = |A_i| (valid sources
only), value log2(P * ((1 - u) * q + u / P)); NaN for a dropped query and for M = 0."""
import math

import numpy as np

MAX_CELLS = 2048
MAX_BANDWIDTHS = 16
LEAVE = ("image", "scanpath", "scanpath_step")


def _arr(sp):
    a = np.asarray(sp, dtype=np.float64)
    return a.reshape(len(a), -1) if a.size else np.zeros((0, 2))


def cell_of(x, y, frame, shape):
    """(row, col), or None for a dropped fixation"""
    (h, w), (Hm, Wm) = frame, shape
    if not (math.isfinite(x) and math.isfinite(y)) or x < 0.0 or x >= w or y < 0.0 or y >= h:
        return None
    return min(int(math.floor((y * Hm) / h)), Hm - 1), min(int(math.floor((x * Wm) / w)), Wm - 1)


def axis_args(v, length, n, b):
    """the exponents of a source at v on an axis of n cells"""
    out = []
    for i in range(n):
        d = ((i + 0.5) * length) / n - v
        out.append(-(d * d) / (2.0 * b * b))
    return out


def axis_weights(v, length, n, b):
    a = axis_args(v, length, n, b)
    m = max(a)
    e = [math.exp(ai - m) for ai in a]
    s = 0.0
    for ei in e:
        s = s + ei
    return [ei / s for ei in e]


def cell_kernel(x, y, frame, shape, b):
    """[Hm, Wm]: the cell kernel of a valid source"""
    (h, w), (Hm, Wm) = frame, shape
    wx, wy = axis_weights(x, w, Wm, b), axis_weights(y, h, Hm, b)
    return np.array([[wy[r] * wx[c] for c in range(Wm)] for r in range(Hm)], dtype=np.float64).reshape(Hm, Wm)


def points(scanpaths, image_groups, frame, shape, max_length=None):
    """the fixations that count, in the caller's order: dicts of s, t, g, x, y, cell (None: dropped); and n' per scanpath"""
    pts, n = [], []
    for s, (sp, g) in enumerate(zip(scanpaths, image_groups)):
        sp = _arr(sp)
        m = len(sp) if max_length is None else min(len(sp), max_length)
        n.append(m)
        for t in range(m):
            x, y = float(sp[t, 0]), float(sp[t, 1])
            pts.append(dict(s=s, t=t, g=int(g), x=x, y=y, cell=cell_of(x, y, frame, shape)))
    return pts, n


def _member(leave, i, j):
    if leave == "image":
        return j["g"] != i["g"]
    if leave == "scanpath":
        return j["g"] == i["g"] and j["s"] != i["s"]
    return j["g"] == i["g"] and j["s"] != i["s"] and j["t"] == i["t"]


def bits(total, M, P, u):
    v = P * ((1.0 - u) * (total / M) + u / P)
    return math.log2(v) if v > 0.0 else -math.inf                  # no epsilon: a zero density scores -inf


def leave_out(scanpaths, image_groups, frame, shape, bandwidth, uniform_mix, leave, max_length=None):
    """plain loops -> {"LL": [S, Tmax], "others": [S, Tmax], "n": [S], "dropped": [S]}"""
    assert leave in LEAVE
    pts, n = points(scanpaths, image_groups, frame, shape, max_length)
    S, Tmax, P = len(n), max(n, default=0), shape[0] * shape[1]
    LL, others = np.full((S, Tmax), np.nan), np.zeros((S, Tmax), dtype=np.int32)
    dropped = np.zeros(S, dtype=np.int32)
    kern = [cell_kernel(p["x"], p["y"], frame, shape, bandwidth) if p["cell"] else None for p in pts]
    for i in pts:
        total, M = 0.0, 0
        for j, kj in zip(pts, kern):
            if j["cell"] and _member(leave, i, j):
                M += 1
                if i["cell"]:
                    total = total + kj[i["cell"]]
        others[i["s"], i["t"]] = M
        if not i["cell"]:
            dropped[i["s"]] += 1
        elif M:
            LL[i["s"], i["t"]] = bits(total, M, P, uniform_mix)
    return dict(LL=LL, others=others, n=np.array(n, dtype=np.int32), dropped=dropped)


def baselines(scanpaths, image_groups, frame, shape, bandwidth, max_length=None):
    """plain loops -> [G, P], G = max(image_groups) + 1: row g = the sum of the kernels of the valid fixations of the other images"""
    pts, _ = points(scanpaths, image_groups, frame, shape, max_length)
    G = max((int(g) for g in image_groups), default=-1) + 1
    out = np.zeros((G,) + tuple(shape))
    for j in pts:
        if j["cell"]:
            kj = cell_kernel(j["x"], j["y"], frame, shape, bandwidth)
            for g in range(G):
                if g != j["g"]:
                    out[g] = out[g] + kj
    return out.reshape(G, -1)


# ---- the quick form: the same definitions, vectorised ------------------------------------------------------------------------------------
class Quick:
    """the fixations that count as arrays (caller's order), and the axis weights of all of them at one bandwidth"""

    def __init__(self, scanpaths, image_groups, frame, shape, max_length=None):
        self.frame, self.shape = (float(frame[0]), float(frame[1])), (int(shape[0]), int(shape[1]))
        (h, w), (Hm, Wm) = self.frame, self.shape
        arrs = [_arr(sp)[:max_length, :2] for sp in scanpaths]
        self.n = np.array([len(a) for a in arrs], dtype=np.int32)
        self.S, self.Tmax = len(arrs), int(self.n.max()) if len(arrs) else 0
        xy = np.concatenate([a for a in arrs if len(a)] or [np.zeros((0, 2))], 0)
        self.x, self.y = xy[:, 0], xy[:, 1]
        self.s = np.repeat(np.arange(self.S), self.n)
        self.t = np.concatenate([np.arange(m) for m in self.n] or [np.zeros(0, dtype=np.int64)]).astype(np.int64)
        self.g = np.repeat(np.asarray(list(image_groups), dtype=np.int64).reshape(-1), self.n)
        self.G = int(max((int(v) for v in image_groups), default=-1)) + 1
        with np.errstate(invalid="ignore"):
            self.ok = np.isfinite(self.x) & np.isfinite(self.y) & (self.x >= 0) & (self.x < w) & (self.y >= 0) & (self.y < h)
            xs, ys = np.where(self.ok, self.x, 0.0), np.where(self.ok, self.y, 0.0)
            self.col = np.minimum(np.floor((xs * Wm) / w).astype(np.int64), Wm - 1)
            self.row = np.minimum(np.floor((ys * Hm) / h).astype(np.int64), Hm - 1)
        self.xs, self.ys = xs, ys

    def axis(self, v, length, n, b):
        """(args [N, n], weights [N, n])"""
        d = ((np.arange(n) + 0.5) * length) / n - v[:, None]
        a = -(d * d) / (2.0 * b * b)
        e = np.exp(a - a.max(1, keepdims=True))
        return a, e / e.sum(1, keepdims=True)

    def weights(self, b):
        (h, w), (Hm, Wm) = self.frame, self.shape
        return self.axis(self.xs, w, Wm, b)[1], self.axis(self.ys, h, Hm, b)[1]

    def exponent_args(self, b):
        """every exponent argument (already minus its maximum) of the valid sources: for the underflow condition of the tests"""
        (h, w), (Hm, Wm) = self.frame, self.shape
        ax, ay = self.axis(self.xs[self.ok], w, Wm, b)[0], self.axis(self.ys[self.ok], h, Hm, b)[0]
        return np.concatenate([(ax - ax.max(1, keepdims=True)).ravel(), (ay - ay.max(1, keepdims=True)).ravel()])

    def own_tables(self, b):
        """[G, Hm, Wm]: the kernels of every image's valid sources, summed"""
        wx, wy = self.weights(b)
        out = np.zeros((self.G,) + self.shape)
        for g in range(self.G):
            m = self.ok & (self.g == g)
            out[g] = wy[m].T @ wx[m]
        return out

    def baselines(self, b):
        own = self.own_tables(b)
        zero = np.zeros_like(own[:1])                                            # exclusive running sums: nothing is subtracted
        before = np.concatenate([zero, np.cumsum(own[:-1], 0)], 0)
        after = np.concatenate([zero, np.cumsum(own[:0:-1], 0)], 0)[::-1]
        return (before + after).reshape(self.G, -1)

    def sums(self, b, leave):
        """(the kernel sum at every query's cell, M) over the points"""
        N = len(self.x)
        total, M = np.zeros(N), np.zeros(N, dtype=np.int64)
        if leave == "image":
            base = self.baselines(b).reshape((self.G,) + self.shape)
            count = np.bincount(self.g[self.ok], minlength=self.G)
            return base[self.g, self.row, self.col], count.sum() - count[self.g]
        wx, wy = self.weights(b)
        for g in np.unique(self.g):
            q = np.flatnonzero(self.g == g)
            src = q[self.ok[q]]
            k = wy[src][:, self.row[q]] * wx[src][:, self.col[q]]                     # [sources, queries]
            member = self.s[src][:, None] != self.s[q][None, :]
            if leave == "scanpath_step":
                member &= self.t[src][:, None] == self.t[q][None, :]
            total[q], M[q] = (k * member).sum(0), member.sum(0)
        return total, M

    def scatter(self, v, fill, dtype):
        out = np.full((self.S, self.Tmax), fill, dtype=dtype)
        out[self.s, self.t] = v
        return out

    def leave_out(self, b, u, leave):
        P = self.shape[0] * self.shape[1]
        total, M = self.sums(b, leave)
        scored = self.ok & (M > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            ll = np.where(scored, np.log2(P * ((1.0 - u) * (total / np.maximum(M, 1)) + u / P)), np.nan)
        return dict(LL=self.scatter(ll, np.nan, np.float64), others=self.scatter(M, 0, np.int32), n=self.n.copy(),
                    dropped=np.bincount(self.s[~self.ok], minlength=self.S).astype(np.int32))


def quick_leave_out(scanpaths, image_groups, frame, shape, bandwidth, uniform_mix, leave, max_length=None):
    assert leave in LEAVE
    return Quick(scanpaths, image_groups, frame, shape, max_length).leave_out(bandwidth, uniform_mix, leave)


def quick_baselines(scanpaths, image_groups, frame, shape, bandwidth, max_length=None):
    return Quick(scanpaths, image_groups, frame, shape, max_length).baselines(bandwidth)


def pooled(LL):
    """(sum, count) of the scored (non-NaN) values of LL; the sum is the correctly rounded one (math.fsum); -inf is a score"""
    v = LL[~np.isnan(LL)]
    return (-math.inf if np.isneginf(v).any() else math.fsum(v.tolist())), int(v.size)


def search(scanpaths, image_groups, frame, shape, bandwidths, uniform_mix, leave, max_length=None, quick=True):
    """the bandwidth search: mean bits of every bandwidth over the scored fixations, and the best one (the first on a tie)"""
    q = Quick(scanpaths, image_groups, frame, shape, max_length) if quick else None
    sums, count = [], 0
    for b in bandwidths:
        res = q.leave_out(b, uniform_mix, leave) if quick else leave_out(scanpaths, image_groups, frame, shape, b, uniform_mix, leave,
                                                                        max_length)
        s, count = pooled(res["LL"])
        sums.append(s)
    sums = np.array(sums, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        means = sums / count if count else np.full(len(sums), np.nan)
    best = float(bandwidths[int(np.argmax(means))]) if count and not np.isnan(means).all() else float("nan")
    return dict(bandwidths=np.asarray(bandwidths, dtype=np.float64), LL=means, sum=sums, count=count, best=best)


# ---- the device's summation order, restated on the host: how far may two correct orders differ? -----------------------------------------
def strided_butterfly_sum(v, lanes=64):
    """lane l adds v[l], v[l + lanes], .. in that order; the partial sums combine by the xor butterfly lanes/2, .., 1"""
    part = [0.0] * lanes
    for i, x in enumerate(v):
        part[i % lanes] = part[i % lanes] + x
    o = lanes // 2
    while o:
        part = [part[l] + part[l ^ o] for l in range(lanes)]
        o //= 2
    return part[0]
