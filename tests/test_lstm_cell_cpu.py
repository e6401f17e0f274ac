"""The restatement of the ConvLSTM cell in tests/lstm_cell_ref.py, without a GPU: anchored to oracle.scanpath_oracle.conv_lstm (forward and every
gradient, fp64, 1e-12), and the conditions of its input builders that the GPU cases of tests/test_lstm_cell_gpu.py rely on -- the stress
inputs hold every listed magnitude in every gate and keep the ref32 / ref64 bar below 1e-4; the hand-built rows attain each term of the
cell backward's documented bound exactly."""
import pytest
import torch
import torch.nn.functional as TF

import lstm_cell_ref as R
from parity import stress_bar

GATES = ("input", "forget", "output")
STREAMS = ["_pos", "_neg"]


def _rel(a, b):
    return (a - b).abs().max().item() / max(1.0, b.abs().max().item())


def test_restatement_matches_the_oracle_conv_lstm():
    """B = 2, 3 x 4 map, C = 4, two streams: the cell behind its convolutions, with the rank-1 term as spcol x wc^T (im2col of the spatial
    maps; per-sample filters contracted with the semantic vectors, flattened as test_ops_gpu.test_lstm_cell_and_gate_conv does)"""
    from oracle import scanpath_oracle as O
    B, Hm, Wm, C, Cx, S, KP = 2, 3, 4, 4, 5, 2, 20
    P = Hm * Wm
    d = lambda *s, seed, scale=1.0: R.randn(*s, seed=seed, scale=scale).double().requires_grad_(True)
    sd, k = {}, 0
    for g in GATES + ("memory",):
        for src, ci in (("x", Cx), ("h", C)):
            sd[f"lstm.{g}_{src}.weight"], sd[f"lstm.{g}_{src}.bias"] = d(C, ci, 3, 3, seed=k, scale=0.3), d(C, seed=k + 1, scale=0.3)
            k += 2
    for g in GATES:
        for sfx in STREAMS:
            sd[f"lstm.{g}{sfx}.weight"], sd[f"lstm.{g}{sfx}.bias"] = d(C, C, 3, 3, seed=k, scale=0.3), d(C, seed=k + 1, scale=0.3)
            k += 2
    x, h, c = d(B, Cx, Hm, Wm, seed=100), d(B, C, Hm, Wm, seed=101), d(B, C, Hm, Wm, seed=102)
    spatial, semantic = [d(B, Hm, Wm, seed=110 + s) for s in range(S)], [d(B, C, seed=120 + s) for s in range(S)]
    gh, gc = R.randn(B, C, Hm, Wm, seed=130).double(), R.randn(B, C, Hm, Wm, seed=131).double()
    leaves = [x, h, c] + spatial + semantic + list(sd.values())
    names = ["x", "h", "c"] + [f"spatial{s}" for s in range(S)] + [f"semantic{s}" for s in range(S)] + list(sd)

    h2, (_, c2) = O.conv_lstm(sd, x, (h, c), spatial, semantic, STREAMS)
    ref = torch.autograd.grad((h2 * gh).sum() + (c2 * gc).sum(), leaves)

    rows = lambda t: t.permute(0, 2, 3, 1).reshape(B, P, -1)                            # NCHW -> [B, P, channels]
    order = GATES + ("memory",)
    # xg carries every bias of the gate (x, h and both streams), hg the bias-free h convolution
    wx, wh = torch.cat([sd[f"lstm.{g}_x.weight"] for g in order]), torch.cat([sd[f"lstm.{g}_h.weight"] for g in order])
    bias = torch.cat([sd[f"lstm.{g}_x.bias"] + sd[f"lstm.{g}_h.bias"] + (sum(sd[f"lstm.{g}{sfx}.bias"] for sfx in STREAMS) if g in GATES else 0)
                      for g in order])
    xg, hg = rows(TF.conv2d(x, wx, bias, padding=1)), rows(TF.conv2d(h, wh, None, padding=1))
    cols, parts = [], []
    for s, sfx in enumerate(STREAMS):
        cols.append(TF.unfold(spatial[s][:, None], 3, padding=1).transpose(1, 2))       # [B, P, 9]
        wr = torch.cat([sd[f"lstm.{g}{sfx}.weight"] for g in GATES])                    # [3C, C, 3, 3]
        wflat = wr.permute(0, 2, 3, 1).reshape(3 * C * 9, C)
        parts.append((semantic[s] @ wflat.t()).view(B, 3 * C, 9))
    spcol = torch.cat(cols + [torch.zeros(B, P, KP - 9 * S, dtype=torch.float64)], 2)
    wc = torch.cat(parts + [torch.zeros(B, 3 * C, KP - 9 * S, dtype=torch.float64)], 2)
    gates, cn, hn = R.cell_apply(R.cell_pre(xg, hg, spcol, wc), rows(c))
    got = torch.autograd.grad((hn * rows(gh)).sum() + (cn * rows(gc)).sum(), leaves)
    assert _rel(hn, rows(h2)) <= 1e-12 and _rel(cn, rows(c2)) <= 1e-12
    for name, a, b in zip(names, got, ref):
        assert float(b.abs().max()) > 0.0, name
        assert _rel(a, b) <= 1e-12, (name, _rel(a, b))

    # cell(): the same numbers from detached inputs, and its gradients = autograd's at the cell's own inputs
    ins = [t.detach() for t in (xg, hg, rows(c), spcol, wc)]
    out = R.cell(*ins, dh=rows(gh), dc=rows(gc))
    lv = [t.clone().requires_grad_(True) for t in ins]
    g2, c3, h3 = R.cell_apply(R.cell_pre(lv[0], lv[1], lv[3], lv[4]), lv[2])
    gr = torch.autograd.grad((h3 * rows(gh)).sum() + (c3 * rows(gc)).sum(), lv)
    assert torch.equal(out["h"], hn.detach()) and torch.equal(out["c"], cn.detach()) and torch.equal(out["gates"], gates.detach())
    for key, b in zip(("dxg", "dhg", "dc_prev", "dspcol", "dwc"), gr):
        assert _rel(out[key], b) <= 1e-12, key
    assert torch.equal(out["dpre"], out["dxg"])
    # the backward from saved gates and the filter gradient on its own
    dpre, dcp = R.cell_backward_from_saved(out["gates"], ins[2], out["c"], rows(gh), rows(gc))
    assert _rel(dpre, out["dpre"]) <= 1e-12 and _rel(dcp, out["dc_prev"]) <= 1e-12
    assert _rel(R.rank1_dwc(out["dpre"], ins[3], 3 * C), out["dwc"]) <= 1e-12


@pytest.mark.parametrize("absent", ["", "hg", "c_prev", "dh", "dc", "hg c_prev dh"])
def test_restatement_with_optional_inputs_absent_equals_zero_inputs(absent):
    rows, C = 5, 4
    t = {"xg": R.randn(rows, 4 * C, seed=1), "hg": R.randn(rows, 4 * C, seed=2), "c_prev": R.randn(rows, C, seed=3),
         "dh": R.randn(rows, C, seed=4), "dc": R.randn(rows, C, seed=5)}
    zeroed = {k: (torch.zeros_like(v) if k in absent.split() else v) for k, v in t.items()}
    none = {k: (None if k in absent.split() else v) for k, v in t.items()}
    a = R.cell(zeroed["xg"], zeroed["hg"], zeroed["c_prev"], dh=zeroed["dh"], dc=zeroed["dc"])
    b = R.cell(none["xg"], none["hg"], none["c_prev"], dh=none["dh"], dc=none["dc"])
    for k in ("gates", "c", "h", "dpre"):
        assert torch.equal(a[k], b[k]), k
    d1 = R.cell_backward_from_saved(a["gates"], zeroed["c_prev"], a["c"], zeroed["dh"], zeroed["dc"])
    d2 = R.cell_backward_from_saved(a["gates"], none["c_prev"], a["c"], none["dh"], none["dc"])
    assert torch.equal(d1[0], d2[0]) and _rel(d1[0], a["dpre"]) <= 1e-12
    assert torch.equal(d1[1], d2[1]) and _rel(d1[1], a["dc_prev"]) <= 1e-12          # an absent c_prev: the gradient at the zero state
    z = R.cell_backward_from_saved(a["gates"], t["c_prev"], a["c"], None, None)
    assert float(z[0].abs().max()) == 0.0 and float(z[1].abs().max()) == 0.0


@pytest.mark.parametrize("rows,C", [(3, 12), (5, 64), (195, 64)])
def test_stress_inputs_hold_every_magnitude_and_keep_the_bar_below_1e_4(rows, C):
    """the saturation cases of the GPU file: every value of STRESS_VALUES in every gate, N(0, 1) entries among them, |c_prev| <= 17 with both
    ends present; the bar max(bar, 10 max|ref32 - ref64|) of every forward and backward output stays below 1e-4, so the inputs cannot
    inflate it until it hides a defect.  (195, 64) = B 3 x P 65 of the rank-1 case, with its rank-1 term.)"""
    xg, cp = R.stress_inputs(rows, C, seed=rows)
    for gate in range(4):
        col = xg[:, gate * C:(gate + 1) * C]
        for v in R.STRESS_VALUES:
            assert bool((col == v).any()), (gate, v)
        other = ~torch.isin(col, torch.tensor(R.STRESS_VALUES))
        assert bool(other.any()) and float(col[other].abs().max()) < 6.0
    assert float(cp.abs().max()) == R.STRESS_CPREV and float(cp.max()) == 17.0 and float(cp.min()) == -17.0
    dh, dc = R.randn(rows, C, seed=7), R.randn(rows, C, seed=8)
    sp = wc = None
    if rows == 195:
        B, P, KP = 3, 65, 20
        xg, cp, dh, dc = xg.view(B, P, 4 * C), cp.view(B, P, C), dh.view(B, P, C), dc.view(B, P, C)
        sp, wc = R.randn(B, P, KP, seed=9), R.randn(B, 3 * C, KP, seed=10, scale=0.2)
    r64 = R.cell(xg, None, cp, sp, wc, dh=dh, dc=dc)
    r32 = R.cell(xg, None, cp, sp, wc, dh=dh, dc=dc, dtype=torch.float32)
    worst = 0.0
    for k, base in (("gates", 3e-6), ("c", 3e-6), ("h", 3e-6), ("dpre", 1e-5), ("dc_prev", 1e-5)):
        assert bool(torch.isfinite(r32[k]).all()) and bool(torch.isfinite(r64[k]).all()), k
        worst = max(worst, stress_bar(base, r32[k], r64[k]))
    # the backward as the kernel runs it: from the saved fp32 gates
    for dt in (torch.float32, torch.float64):
        assert all(bool(torch.isfinite(t).all()) for t in R.cell_backward_from_saved(r32["gates"], cp, r32["c"], dh, dc, dtype=dt))
    b32 = R.cell_backward_from_saved(r32["gates"], cp, r32["c"], dh, dc, dtype=torch.float32)
    b64 = R.cell_backward_from_saved(r32["gates"], cp, r32["c"], dh, dc)
    worst = max(worst, stress_bar(1e-5, b32[0], b64[0]), stress_bar(1e-5, b32[1], b64[1]))
    print(f"stress bar rows={rows} C={C}: worst {worst:.2e}")
    assert worst < 1e-4, worst


@pytest.mark.parametrize("c_bound,cprev_bound", [(1.0, 0.0), (17.0, 16.0)])
@pytest.mark.parametrize("a_dh,a_dc", [(1.0, 1.0), (1.5, 2.0 ** -7), (0.0, 2.0)])
def test_hand_built_rows_attain_each_term_of_the_documented_bound(c_bound, cprev_bound, a_dh, a_dc):
    """|d_o| = max|dh| c_bound / 4, |d_f| = D cprev_bound / 4 and |d_g| = D are reached exactly by the rows built for them, the inputs keep
    the maxima they are declared with, and no entry of dpre exceeds the bound (fp64)"""
    C = 256
    gates, c_prev, c_out, dh, dc = R.bound_attained_inputs(C, c_bound, cprev_bound, a_dh, a_dc)
    assert float(dh.abs().max()) == a_dh and float(dc.abs().max()) == a_dc
    assert float(c_out.abs().max()) == c_bound and float(c_prev.abs().max()) == cprev_bound
    assert 0.0 <= float(gates[:, :3 * C].min()) and float(gates[:, :3 * C].max()) <= 1.0 and float(gates[:, 3 * C:].abs().max()) < 1.0
    dpre, _ = R.cell_backward_from_saved(gates, c_prev, c_out, dh, dc)
    D = float(dh.abs().max().double() + dc.abs().max().double())
    assert float(dpre[0, 2 * C:3 * C].abs().max()) == a_dh * c_bound / 4
    assert float(dpre[1, C:2 * C].abs().max()) == D * cprev_bound / 4
    assert float(dpre[2, 3 * C:].abs().max()) == D
    bound = R.documented_bound(a_dh, a_dc, c_bound, cprev_bound)
    assert float(dpre.abs().max()) == bound
