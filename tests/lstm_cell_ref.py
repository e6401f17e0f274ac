"""Plain torch restatement of the ConvLSTM cell (AiR/models/baseline_attention.py:37-56 behind its convolutions), the reference side of
tests/test_lstm_cell_cpu.py and tests/test_lstm_cell_gpu.py.  Layout of the HIP kernels: rows = (sample, pixel), gate-major channels
[i | f | o | g] of width C each.

    pre = xg (+ hg) (+ spcol x wc^T on the i, f, o gates);  i, f, o = sigmoid, g = tanh;  c' = f c + i g;  h' = o c'   (no tanh on the cell)

dtype is a parameter (fp64 by default; fp32 for the ref32 side of a stress bar).  Nothing here touches a GPU: test_lstm_cell_cpu.py anchors
these lines to oracle.scanpath_oracle.conv_lstm at 1e-12, and holds the input builders below to the conditions the GPU cases rely on."""
import numpy as np
import torch

STRESS_VALUES = (100.0, -100.0, 88.0, -88.0, 20.0, -20.0, 1e-3, -1e-3, 0.0)
STRESS_CPREV = 17.0


def _leaf(t, dtype):
    return None if t is None else t.detach().clone().to(dtype).requires_grad_(True)


def _gen(seed):
    return np.random.Generator(np.random.PCG64(seed))


def randn(*shape, seed=0, scale=1.0):
    return torch.from_numpy(_gen(seed).standard_normal(shape).astype(np.float32) * scale)


def cell_pre(xg, hg=None, spcol=None, wc=None):
    """pre-activations [..., 4C]; the rank-1 term (xg [B, P, 4C], spcol [B, P, KP], wc [B, 3C, KP]) reaches the i, f, o gates only"""
    pre = xg if hg is None else xg + hg
    if spcol is not None:
        r1 = torch.bmm(spcol, wc.transpose(1, 2))                                   # [B, P, 3C]
        pre = pre + torch.cat([r1, torch.zeros_like(pre[..., :pre.shape[-1] // 4])], -1)
    return pre


def cell_apply(pre, c_prev=None):
    """(gates [..., 4C] activated, c', h')"""
    C = pre.shape[-1] // 4
    i, f, o, g = pre[..., :C].sigmoid(), pre[..., C:2 * C].sigmoid(), pre[..., 2 * C:3 * C].sigmoid(), pre[..., 3 * C:].tanh()
    c = i * g if c_prev is None else f * c_prev + i * g
    return torch.cat([i, f, o, g], -1), c, o * c


def cell(xg, hg=None, c_prev=None, spcol=None, wc=None, dh=None, dc=None, dtype=torch.float64):
    """forward, and with dh / dc (either may be None = 0) every input gradient through autograd.  Returns a dict: pre, gates, c, h and --
    when a cotangent is given -- dpre, dxg (= dpre), dhg, dc_prev, dspcol, dwc (None for an absent input)."""
    L = {k: _leaf(v, dtype) for k, v in (("xg", xg), ("hg", hg), ("c_prev", c_prev), ("spcol", spcol), ("wc", wc))}
    pre = cell_pre(L["xg"], L["hg"], L["spcol"], L["wc"])
    pre.retain_grad()
    gates, c, h = cell_apply(pre, L["c_prev"])
    out = {"pre": pre.detach(), "gates": gates.detach(), "c": c.detach(), "h": h.detach()}
    if dh is None and dc is None:
        return out
    tot = 0.0
    if dh is not None:
        tot = tot + (h * dh.to(dtype)).sum()
    if dc is not None:
        tot = tot + (c * dc.to(dtype)).sum()
    tot.backward()
    out["dpre"] = pre.grad
    for k in L:
        out["d" + k] = None if L[k] is None else L[k].grad
    return out


def cell_backward_from_saved(gates, c_prev, c_out, dh=None, dc=None, dtype=torch.float64):
    """(dpre [..., 4C], dc_prev) of the cell from its SAVED activated gates and cell state, the form the backward kernel works from: autograd
    over c' = f c + i g, h' = o c' with the gates as leaves, times the local derivatives s (1 - s) and 1 - g^2 written in the outputs.
    c_out takes the place of the recomputed c' as a value (it is what o's gradient multiplies); the gradient flows through f c + i g.
    c_prev = None is a zero state: dc_prev is then the gradient at that zero state (dc' f), as the kernel writes it."""
    C = gates.shape[-1] // 4
    gl = _leaf(gates, dtype)
    cp = _leaf(torch.zeros_like(c_out) if c_prev is None else c_prev, dtype)
    i, f, o, g = gl[..., :C], gl[..., C:2 * C], gl[..., 2 * C:3 * C], gl[..., 3 * C:]
    c = f * cp + i * g
    c = c + (c_out.to(dtype) - c).detach()
    h = o * c
    if dh is None and dc is None:
        return torch.zeros_like(gl), torch.zeros_like(c)
    tot = 0.0
    if dh is not None:
        tot = tot + (h * dh.to(dtype)).sum()
    if dc is not None:
        tot = tot + (c * dc.to(dtype)).sum()
    tot.backward()
    gd = gates.detach().to(dtype)
    local = torch.cat([gd[..., :3 * C] * (1 - gd[..., :3 * C]), 1 - gd[..., 3 * C:] ** 2], -1)
    return gl.grad * local, cp.grad


def rank1_dwc(dpre, spcol, N3, dtype=torch.float64):
    """dwc [B, N3, KP] = dpre[b][:, :N3]^T x spcol[b]"""
    return torch.bmm(dpre[..., :N3].to(dtype).transpose(1, 2), spcol.to(dtype))


# ====================================================================================================================
# input builders shared by the CPU conditions and the GPU cases
# ====================================================================================================================
def stress_inputs(rows, C, seed=0):
    """(xg [rows, 4C], c_prev [rows, C]): two thirds of the pre-activations from STRESS_VALUES (every value in every gate), the rest N(0, 1);
    c_prev uniform in [-17, 17] with both ends present"""
    g = _gen(1000 + seed)
    n = rows * 4 * C
    vals = np.array(STRESS_VALUES, np.float32)
    xg = g.standard_normal(n).astype(np.float32)
    pick = g.integers(0, 3 * len(vals) // 2 + 1, n)                  # < len(vals): that stress value; else keep the normal entry
    xg = np.where(pick < len(vals), vals[np.minimum(pick, len(vals) - 1)], xg).astype(np.float32).reshape(rows, 4 * C)
    for gate in range(4):                                            # every value in every gate, whatever the draw
        for k, v in enumerate(vals):
            xg[(gate * len(vals) + k) % rows, gate * C + (k % C)] = v
    cp = g.uniform(-STRESS_CPREV, STRESS_CPREV, (rows, C)).astype(np.float32)
    cp[0, 0], cp[-1, -1] = STRESS_CPREV, -STRESS_CPREV
    return torch.from_numpy(xg), torch.from_numpy(cp)


def bound_attained_inputs(C, c_bound, cprev_bound, a_dh, a_dc, seed=0):
    """hand-built saved state of 8 rows x C channels that makes each term of the cell backward's documented bound
        max(D, max|dh| c_bound / 4, D cprev_bound / 4),  D = max|dh| + max|dc|
    an equality somewhere: returns (gates, c_prev, c_out, dh, dc) with max|dh| = a_dh, max|dc| = a_dc, |c_out| <= c_bound, |c_prev| <=
    cprev_bound exactly.  Row 0: o = 0.5, c_out = +-c_bound, dh = +-a_dh           -> |d_o| = a_dh c_bound / 4
                          row 1: f = 0.5, o = 1, c_prev = +-cprev_bound, dh = a_dh, dc = a_dc (equal signs) -> |d_f| = D cprev_bound / 4
                          row 2: i = 1, g = 0, o = 1, dh = a_dh, dc = a_dc          -> |d_g| = D
    the other rows: gates uniform in (0, 1) (g in (-1, 1)), states and cotangents uniform inside their bounds."""
    g = _gen(2000 + seed)
    rows = 8
    u = lambda lo, hi, *s: torch.from_numpy(g.uniform(lo, hi, s).astype(np.float32))
    gates = torch.cat([u(0.0, 1.0, rows, 3 * C), u(-1.0, 1.0, rows, C)], 1)
    c_prev, c_out = u(-1.0, 1.0, rows, C) * cprev_bound, u(-1.0, 1.0, rows, C) * c_bound
    dh, dc = u(-1.0, 1.0, rows, C) * a_dh, u(-1.0, 1.0, rows, C) * a_dc
    sign = torch.where(torch.arange(C) % 2 == 0, 1.0, -1.0)
    gates[0, 2 * C:3 * C] = 0.5
    c_out[0], dh[0] = c_bound * sign, a_dh * sign.flip(0)
    gates[1, C:2 * C], gates[1, 2 * C:3 * C] = 0.5, 1.0
    c_prev[1], dh[1], dc[1] = cprev_bound * sign, a_dh * sign, a_dc * sign
    gates[2, :C], gates[2, 2 * C:3 * C], gates[2, 3 * C:] = 1.0, 1.0, 0.0
    dh[2], dc[2] = a_dh * sign, a_dc * sign
    return gates, c_prev, c_out, dh, dc


def documented_bound(a_dh, a_dc, c_bound, cprev_bound):
    D = a_dh + a_dc
    return max(D, 0.25 * a_dh * c_bound, 0.25 * D * cprev_bound)
