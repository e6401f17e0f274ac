"""The ConvLSTM cell kernels -- lstm_fwd_kernel, lstm_rank1_fwd_kernel, rank1_dwc_kernel, lstm_bwd_kernel of csrc/decoder.hip through the ctypes ABI,
and the cell epilogue of sp_gateconv_lstm_f16x2 (csrc/conv_f16x2.hip) through scanpaths_amd.functional -- against the plain fp64 restatement of
tests/lstm_cell_ref.py (anchored to the oracle by tests/test_lstm_cell_cpu.py), at the shapes where their loops change path: a partial wave, the
grid-stride loop behind 2048 blocks, 64-pixel tiles and 256-pixel blocks / chunks less one / exactly / plus one, every tap count of the LDS passes,
absent optional inputs, dead samples (row_last) whose inputs hold NaN, saturated gates, and the 2xfp16 operand of the gate gradient with its bound.

Bars: those tests/test_ops_gpu.py::test_lstm_cell_and_gate_conv holds these ops to, same metric (parity.close): 3e-6 for gates / c / h, 1e-5 for every
gradient; saturation cases max(that bar, 10 x max|ref32 - ref64|) of the restatement (tests/test_lstm_cell_cpu.py keeps that below 1e-4).  The
planes bar (2^-21 x bound), the exact max|.| words and the bit-equalities are conditions.  Every test prints its worst err / bar
(profiles/lstm_cell_parity.md)."""
import functools
import itertools
import math

import pytest
import torch
import torch.nn.functional as TF

import lstm_cell_ref as R
from parity import NAN, Worst, abi as _abi, decode_split as _decode_split, dev as _dev, rand as _rand, stress_bar

pytestmark = pytest.mark.gpu

# ====================================================================================================================
# the ABI, with every output poisoned and every max|.| word zeroed by the caller
# ====================================================================================================================
def _d(t):
    return None if t is None else t.contiguous().to(_dev())


def _bits(v):
    """a device word holding the float bits of v"""
    return torch.tensor([v], dtype=torch.float32, device=_dev()).view(torch.int32)


def _word_value(w):
    return float(w.view(torch.float32)[0])


def _fwd(xg, hg, cp):
    """sp_lstm_pointwise_fwd on [rows, 4C] -> (gates, c, h) on the device"""
    hip, L = _abi()
    rows, C = xg.shape[0], xg.shape[1] // 4
    xg, hg, cp = _d(xg), _d(hg), _d(cp)
    gates, c, h = torch.full_like(xg, NAN), torch.full((rows, C), NAN, device=xg.device), torch.full((rows, C), NAN, device=xg.device)
    rc = L.sp_lstm_pointwise_fwd(hip.ptr(xg), hip.ptr(hg), hip.ptr(cp), rows, C, hip.ptr(gates), hip.ptr(c), hip.ptr(h), hip.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return gates, c, h


def _rank1_fwd(xg, hg, cp, sp, wc):
    """sp_lstm_rank1_fwd on xg [B, P, 4C] -> (rc, gates, c, h, max|h| word as a float)"""
    hip, L = _abi()
    B, P, C, KP = xg.shape[0], xg.shape[1], xg.shape[2] // 4, sp.shape[2]
    xg, hg, cp, sp, wc = _d(xg), _d(hg), _d(cp), _d(sp), _d(wc)
    gates = torch.full_like(xg, NAN)
    c, h = torch.full((B, P, C), NAN, device=xg.device), torch.full((B, P, C), NAN, device=xg.device)
    word = torch.zeros(1, dtype=torch.int32, device=xg.device)
    rc = L.sp_lstm_rank1_fwd(hip.ptr(xg), hip.ptr(hg), hip.ptr(cp), hip.ptr(sp), hip.ptr(wc), B, P, C, KP, hip.ptr(gates), hip.ptr(c), hip.ptr(h),
                             hip.ptr(word), hip.stream())
    torch.cuda.synchronize()
    return rc, gates, c, h, _word_value(word)


def _dwc(dpre, sp, N3):
    """sp_rank1_dwc on dpre [B, P, ld], spcol [B, P, KP]; workspace and result pre-filled with NaN"""
    hip, L = _abi()
    B, P, ld = dpre.shape
    KP = sp.shape[2]
    dpre, sp = _d(dpre), _d(sp)
    nbytes = L.sp_rank1_dwc_workspace(B, P, N3, KP)
    assert nbytes == ((P + 255) // 256) * B * N3 * KP * 4
    ws = torch.full((nbytes // 4,), NAN, device=dpre.device)
    out = torch.full((B, N3, KP), NAN, device=dpre.device)
    rc = L.sp_rank1_dwc(hip.ptr(dpre), hip.ptr(sp), B, P, ld, N3, KP, hip.ptr(ws), hip.ptr(out), hip.stream())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out


def _bwd(dh, dc, gates, cp, c, *, planes=False, dh_amax=None, dc_amax=None, c_bound=0.0, cprev_bound=0.0, last=None, step=0, rps=1, want_rc=False):
    """sp_lstm_pointwise_bwd on device tensors [rows, .]; outputs (and the planes with their 32 trailing halves) pre-filled with NaN, the two
    max|.| words zeroed here"""
    hip, L = _abi()
    dev = gates.device
    rows, C = gates.shape[0], gates.shape[1] // 4
    dpre, dcp = torch.full_like(gates, NAN), torch.full((rows, C), NAN, device=dev)
    w_dpre, w_dcp = torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    pl = torch.full((2 * rows * 4 * C + 32,), NAN, dtype=torch.float16, device=dev) if planes else None
    scale = torch.zeros(2, device=dev) if planes else None
    a_dh = _bits(dh_amax) if dh_amax is not None else None
    a_dc = _bits(dc_amax) if dc_amax is not None else None
    rc = L.sp_lstm_pointwise_bwd(hip.ptr(dh), hip.ptr(dc), hip.ptr(gates), hip.ptr(cp), hip.ptr(c), rows, C, hip.ptr(dpre), hip.ptr(dcp),
                                 hip.ptr(w_dpre), hip.ptr(w_dcp), hip.ptr(a_dh), hip.ptr(a_dc), c_bound, cprev_bound, hip.ptr(pl), hip.ptr(scale),
                                 hip.ptr(last), step, rps, hip.stream())
    torch.cuda.synchronize()
    if want_rc:
        return rc
    assert rc == 0, rc
    return {"dpre": dpre, "dcp": dcp, "dpre_amax": _word_value(w_dpre), "dcp_amax": _word_value(w_dcp), "planes": pl, "scale": scale}


def _amax(t):
    return float(t.abs().max()) if t is not None and t.numel() else 0.0


# ====================================================================================================================
# 1, 4: the pointwise cell, forward and backward
# ====================================================================================================================
PLAIN_SHAPES = [(1, 4), (3, 12), (5, 64), (2049, 1024)]      # one quad; 9 quads: a partial wave; 80 quads; 524 544 quads > 2048 blocks x 256 threads
SMALL = PLAIN_SHAPES[:2]


@functools.lru_cache(maxsize=None)
def _plain_inputs(rows, C):
    return {"xg": _rand(rows, 4 * C, seed=1), "hg": _rand(rows, 4 * C, seed=2), "cp": _rand(rows, C, seed=3), "dh": _rand(rows, C, seed=4),
            "dc": _rand(rows, C, seed=5)}


@functools.lru_cache(maxsize=None)
def _plain_state(rows, C, has_hg, has_cp):
    """the kernel's forward on the shared inputs and the fp64 forward, computed once per (shape, presence) and left unchanged"""
    t = _plain_inputs(rows, C)
    hg, cp = (t["hg"] if has_hg else None), (t["cp"] if has_cp else None)
    return _fwd(t["xg"], hg, cp), R.cell(t["xg"], hg, cp)


@functools.lru_cache(maxsize=None)
def _plain_backward_ref(rows, C):
    """fp64 backward from the kernel's own saved gates / c_out with both cotangents and c_prev present (shared by the plain and the planes case)"""
    t = _plain_inputs(rows, C)
    (gates, c, _), _ = _plain_state(rows, C, True, True)
    return R.cell_backward_from_saved(gates.cpu(), t["cp"], c.cpu(), t["dh"], t["dc"])


@pytest.mark.parametrize("rows,C", PLAIN_SHAPES)
def test_pointwise_forward_at_edge_shapes(rows, C):
    """lstm_fwd_kernel: gates, c', h' against fp64; hg / c_prev present or NULL in all four combinations at the two small shapes"""
    w = Worst(f"lstm_pointwise_fwd rows={rows} C={C}")
    combos = list(itertools.product((True, False), repeat=2)) if (rows, C) in SMALL else [(True, True)]
    for has_hg, has_cp in combos:
        (gates, c, h), ref = _plain_state(rows, C, has_hg, has_cp)
        tag = f"hg={'yes' if has_hg else 'NULL'} c_prev={'yes' if has_cp else 'NULL'}"
        w.close(gates, ref["gates"], 3e-6, f"gates ({tag})")
        w.close(c, ref["c"], 3e-6, f"c ({tag})")
        w.close(h, ref["h"], 3e-6, f"h ({tag})")
    w.report()


@pytest.mark.parametrize("rows,C", PLAIN_SHAPES)
def test_pointwise_backward_at_edge_shapes(rows, C):
    """lstm_bwd_kernel without planes: dpre and dc_prev against fp64 autograd of the restatement fed the kernel's own saved gates / c_out; the two
    max|.| words (zeroed here) equal the maxima of the kernel's own outputs exactly.  At (3, 12) every combination of dh / dc / c_prev present
    or NULL; both cotangents NULL give exact zeros."""
    w = Worst(f"lstm_pointwise_bwd rows={rows} C={C}")
    t = _plain_inputs(rows, C)
    combos = list(itertools.product((True, False), repeat=3)) if (rows, C) == (3, 12) else [(True, True, True)]
    for has_dh, has_dc, has_cp in combos:
        (gates, c, _), _ = _plain_state(rows, C, True, has_cp)
        dh, dc, cp = (t["dh"] if has_dh else None), (t["dc"] if has_dc else None), (t["cp"] if has_cp else None)
        res = _bwd(_d(dh), _d(dc), gates, _d(cp), c)
        ref = _plain_backward_ref(rows, C) if (has_dh and has_dc and has_cp) else R.cell_backward_from_saved(gates.cpu(), cp, c.cpu(), dh, dc)
        tag = f"dh={'yes' if has_dh else 'NULL'} dc={'yes' if has_dc else 'NULL'} c_prev={'yes' if has_cp else 'NULL'}"
        w.close(res["dpre"], ref[0], 1e-5, f"dpre ({tag})")
        w.close(res["dcp"], ref[1], 1e-5, f"dc_prev ({tag})")
        assert res["dpre_amax"] == _amax(res["dpre"]) and res["dcp_amax"] == _amax(res["dcp"]), tag
        if not has_dh and not has_dc:
            assert _amax(res["dpre"]) == 0.0 and _amax(res["dcp"]) == 0.0
        else:
            assert _amax(res["dpre"]) > 0.0
    w.report()


# ====================================================================================================================
# 2: the cell with the rank-1 gate term
# ====================================================================================================================
def _rank1_inputs(B, P, C, KP, seed=20):
    """spcol and wc with a magnitude of their own per sample and (wc) per gate, so that a wrong b, g or c0 offset moves the result by far more
    than the bar"""
    xg, hg, cp = _rand(B, P, 4 * C, seed=seed), _rand(B, P, 4 * C, seed=seed + 1), _rand(B, P, C, seed=seed + 2)
    sp, wc = _rand(B, P, KP, seed=seed + 3), _rand(B, 3 * C, KP, seed=seed + 4, scale=1.0 / math.sqrt(KP))
    for b in range(B):
        sp[b] *= 1.0 + 0.5 * b
        wc[b] *= 1.0 - 0.25 * b
    for g, k in enumerate((0.5, 1.0, 1.5)):
        wc[:, g * C:(g + 1) * C] *= k
    return xg, hg, cp, sp, wc


def _rank1_compare(w, xg, hg, cp, sp, wc, tag=""):
    rc, gates, c, h, hmax = _rank1_fwd(xg, hg, cp, sp, wc)
    assert rc == 0, rc
    ref = R.cell(xg, hg, cp, sp, wc)
    w.close(gates, ref["gates"], 3e-6, "gates" + tag)
    w.close(c, ref["c"], 3e-6, "c" + tag)
    w.close(h, ref["h"], 3e-6, "h" + tag)
    assert hmax == _amax(h), (hmax, _amax(h))
    return gates, c, h


@pytest.mark.parametrize("C", [64, 128])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257])
def test_rank1_forward_at_tile_and_block_boundaries(P, C):
    """lstm_rank1_fwd_kernel at B = 3, KP = 20: one pixel, a 64-pixel tile and a 256-pixel block less one / exactly / plus one (the tap staging
    of a partial tile), one and two 64-channel blocks; the max|h| word equals the maximum of the kernel's own h_out"""
    w = Worst(f"lstm_rank1_fwd B=3 P={P} C={C} KP=20")
    _rank1_compare(w, *_rank1_inputs(3, P, C, 20))
    w.report()


@pytest.mark.parametrize("KP", [1, 9, 12, 32, 64])
def test_rank1_forward_at_every_tap_count(KP):
    """(B, P, C) = (1, 65, 64): one tap, one stream, the model's 12, and the documented limit KP = 64 -- 64 x 256 x 4 = 65 536 B of dynamic LDS plus
    16 B static, inside the 160 KiB a single workgroup may declare on gfx950: the launch is legal and the limit of the header stands.  Above it
    the entry point refuses (SP_EINVAL) before any launch."""
    w = Worst(f"lstm_rank1_fwd B=1 P=65 C=64 KP={KP}")
    ins = _rank1_inputs(1, 65, 64, KP, seed=30)
    _rank1_compare(w, *ins)
    if KP == 64:
        xg, hg, cp = ins[:3]
        sp, wc = _rand(1, 65, 65, seed=35), _rand(1, 192, 65, seed=36)
        assert _rank1_fwd(xg, hg, cp, sp, wc)[0] == -1
    w.report()


def test_rank1_forward_without_hg_and_previous_state():
    w = Worst("lstm_rank1_fwd B=3 P=65 C=128 hg / c_prev NULL")
    xg, hg, cp, sp, wc = _rank1_inputs(3, 65, 128, 20, seed=40)
    for has_hg, has_cp in ((False, False), (True, False), (False, True)):
        _rank1_compare(w, xg, hg if has_hg else None, cp if has_cp else None, sp, wc, f" (hg={has_hg} c_prev={has_cp})")
    w.report()


# ====================================================================================================================
# 3: gradient of the contracted rank-1 filters
# ====================================================================================================================
DWC_CASES = ([(2, P, 192, 256, 20) for P in (1, 3, 15, 16, 17, 255, 256, 257, 513)]           # 4 / 16 pixels per wave pass, 256 per chunk
             + [(2, 33, N3, N3 + 4, 20) for N3 in (4, 252, 256, 260)]                           # 256 columns per block
             + [(2, 33, 192, 256, KP) for KP in (1, 5, 6, 7, 12, 18, 24)]                       # 6 taps per LDS pass
             + [(1, 33, 192, 256, 20), (2, 33, 192, 192, 20)])                                  # one sample; no trailing columns


@pytest.mark.parametrize("B,P,N3,ld,KP", DWC_CASES)
def test_rank1_dwc_at_every_loop_boundary(B, P, N3, ld, KP):
    """rank1_dwc_kernel + its fixed-order reduce: dwc[b] = dpre[b][:, :N3]^T x spcol[b] against fp64 bmm.  Columns [N3, ld) of dpre hold NaN and
    the workspace and the result start as NaN: the result must be finite.  Two runs are bit-identical."""
    w = Worst(f"rank1_dwc B={B} P={P} N3={N3} ld={ld} KP={KP}")
    dpre, sp = _rand(B, P, ld, seed=50), _rand(B, P, KP, seed=51)
    dpre[..., N3:] = NAN
    out = _dwc(dpre, sp, N3)
    assert bool(torch.isfinite(out).all())
    w.close(out, R.rank1_dwc(dpre, sp, N3), 1e-5, "dwc")
    assert torch.equal(_dwc(dpre, sp, N3), out)
    w.report()


# ====================================================================================================================
# 5: row_last without planes
# ====================================================================================================================
def _saved_state(B, P, C, seed):
    """device tensors [B * P, .] of one cell step: cotangents, the forward kernel's gates / c_out, c_prev"""
    rows = B * P
    xg, cp = _rand(rows, 4 * C, seed=seed), _rand(rows, C, seed=seed + 1)
    dh, dc = _d(_rand(rows, C, seed=seed + 2)), _d(_rand(rows, C, seed=seed + 3))
    gates, c, _ = _fwd(xg, None, cp)
    return dh, dc, gates, _d(cp), c


def _fill_samples(ts, B, dead, value):
    """copies of the [B * P, n] tensors with every row of the samples `dead` set to value"""
    res = []
    for t in ts:
        u = t.clone()
        u.view(B, -1)[dead] = value
        res.append(u)
    return res


@pytest.mark.parametrize("B,P,C,last", [(5, 3, 4, [2, 1, -1, 5, 0]), (3, 64, 64, [1, 7, -1])])
def test_pointwise_backward_skips_dead_samples(B, P, C, last):
    """lstm_bwd_kernel's row_last branch at row_step = 2 ((5, 3, 4): one wave spans all five samples): samples with last < 2 (and last = -1) get
    exact zeros although all five of their inputs hold NaN; the live samples are bit-equal to the dense launch on zero-filled inputs, the max|.|
    words equal the maxima over the live rows, and dpre of the dense launch matches fp64.  rows % rows_per_sample != 0 is SP_EINVAL."""
    w = Worst(f"lstm_pointwise_bwd row_last B={B} P={P} C={C}")
    step = 2
    state = _saved_state(B, P, C, seed=60)
    lastd = torch.tensor(last, dtype=torch.int32, device=_dev())
    dead = [b for b in range(B) if last[b] < step]
    live = [b for b in range(B) if last[b] >= step]
    assert dead and live and -1 in last
    dense = _bwd(*_fill_samples(state, B, dead, 0.0))
    sparse = _bwd(*_fill_samples(state, B, dead, NAN), last=lastd, step=step, rps=P)
    for k in ("dpre", "dcp"):
        s, dn = sparse[k].view(B, -1), dense[k].view(B, -1)
        assert float(s[dead].abs().max()) == 0.0, k                    # (NaN would fail this comparison too)
        assert torch.equal(s[live], dn[live]), k
        assert sparse[k + "_amax"] == _amax(dn[live]) and _amax(dn[live]) > 0.0, k
    zs = [t.cpu() for t in _fill_samples(state, B, dead, 0.0)]
    ref = R.cell_backward_from_saved(zs[2], zs[3], zs[4], zs[0], zs[1])
    w.close(dense["dpre"], ref[0], 1e-5, "dpre (dense)")
    w.close(dense["dcp"], ref[1], 1e-5, "dc_prev (dense)")
    assert _bwd(*state, last=lastd, step=step, rps=P + 1, want_rc=True) == -1
    w.report()


# ====================================================================================================================
# 6: the 2xfp16 operand of the gate gradient and its bound
# ====================================================================================================================
def _check_planes(res, rows, C):
    """the conditions on the emitted operand; returns (max|decode - dpre| / (2^-21 bound), bound)"""
    from scanpaths_amd import functional as F
    scale, bound = (float(v) for v in res["scale"].cpu())
    dpre, pl, n = res["dpre"], res["planes"], rows * 4 * C
    assert bound >= _amax(dpre), (bound, _amax(dpre))
    assert scale > 0.0 and math.frexp(scale)[0] == 0.5, scale                               # a power of two
    assert 8192.0 <= bound * scale < 16384.0, (bound, scale)
    assert bool(torch.isfinite(pl[:2 * n].float()).all())
    assert float(pl[2 * n:].float().abs().max()) == 0.0                                     # the 64-byte zero block (was NaN)
    dec = _decode_split(F.SplitOperand(pl, res["scale"], "f16x2"), (rows, 4 * C))
    err = float((dec.double() - dpre.double()).abs().max())
    assert err <= 2.0 ** -21 * bound, (err, bound)
    return err / (2.0 ** -21 * bound), bound


def _planes_line(name, worst, n):
    print(f"PARITY {name}: worst err/bar {worst[0]:.3f} ({worst[1]}; bar 2^-21 x bound; {n} launches)")


@pytest.mark.parametrize("rows,C", [(3, 256), (64, 256), (3, 1024), (64, 1024), (2049, 1024)])
def test_backward_planes_decode_to_the_fp32_gate_gradient(rows, C):
    """lstm_bwd_kernel with planes: the bound covers max|dpre| of the fp32 output, the scale is the power of two that puts it into [8192, 16384),
    every half is finite, the planes decode to dpre within 2^-21 x bound and the 32 trailing halves (NaN before) are zero -- with max|dh| /
    max|dc| given exactly and as 2x over-estimates, and (small shapes) with dh and its word NULL.  dpre itself against fp64."""
    w = Worst(f"lstm_pointwise_bwd planes rows={rows} C={C}")
    t = _plain_inputs(rows, C)
    (gates, c, _), _ = _plain_state(rows, C, True, True)
    dh, dc, cp = _d(t["dh"]), _d(t["dc"]), _d(t["cp"])
    cb, cpb = _amax(c), _amax(cp)
    ref = _plain_backward_ref(rows, C)
    worst, runs = (0.0, ""), 0
    for over in ((1.0, 2.0) if rows != 2049 else (1.0,)):
        res = _bwd(dh, dc, gates, cp, c, planes=True, dh_amax=over * _amax(dh), dc_amax=over * _amax(dc), c_bound=cb, cprev_bound=cpb)
        ratio, bound = _check_planes(res, rows, C)
        want = R.documented_bound(over * _amax(dh), over * _amax(dc), cb, cpb)
        assert want <= bound <= want * 1.001, (bound, want)
        worst, runs = max(worst, (ratio, f"maxima x {over:g}")), runs + 1
        w.close(res["dpre"], ref[0], 1e-5, f"dpre (maxima x {over:g})")
        w.close(res["dcp"], ref[1], 1e-5, f"dc_prev (maxima x {over:g})")
    if rows != 2049:
        res = _bwd(None, dc, gates, cp, c, planes=True, dh_amax=None, dc_amax=_amax(dc), c_bound=cb, cprev_bound=cpb)
        ratio, _ = _check_planes(res, rows, C)
        worst, runs = max(worst, (ratio, "dh NULL")), runs + 1
        ref0 = R.cell_backward_from_saved(gates.cpu(), t["cp"], c.cpu(), None, t["dc"])
        w.close(res["dpre"], ref0[0], 1e-5, "dpre (dh NULL)")
    _planes_line(f"lstm_pointwise_bwd planes decode rows={rows} C={C}", worst, runs)
    w.report()


@pytest.mark.parametrize("c_bound,cprev_bound", [(1.0, 0.0), (17.0, 16.0)])
def test_backward_bound_is_attained_and_still_holds(c_bound, cprev_bound):
    """hand-built gates make each term of the documented bound max(D, max|dh| c_bound / 4, D cprev_bound / 4) an equality (lstm_cell_ref.
    bound_attained_inputs; tests/test_lstm_cell_cpu.py checks the construction in fp64), c_bound / cprev_bound passed exactly, at the model's
    t + 1 after the first and the last of 16 steps.  max|dpre| of the kernel reaches the documented value and the reported bound still covers
    it: a bound without its margin, or half of it, fails here."""
    C, rows = 256, 8
    w = Worst(f"lstm_pointwise_bwd bound attained c_bound={c_bound:g} cprev_bound={cprev_bound:g}")
    worst, runs = (0.0, ""), 0
    for a_dh, a_dc in ((1.0, 1.0), (1.5, 2.0 ** -7), (0.0, 2.0)):
        gates, cp, c, dh, dc = (_d(t) for t in R.bound_attained_inputs(C, c_bound, cprev_bound, a_dh, a_dc))
        res = _bwd(dh, dc, gates, cp, c, planes=True, dh_amax=a_dh, dc_amax=a_dc, c_bound=c_bound, cprev_bound=cprev_bound)
        want = R.documented_bound(a_dh, a_dc, c_bound, cprev_bound)
        got = _amax(res["dpre"])
        assert abs(got - want) <= 1e-6 * want, (got, want)                       # the rows built for it attain the dominant term
        ratio, bound = _check_planes(res, rows, C)                               # ... and bound >= max|dpre| with it
        assert bound <= want * 1.001, (bound, want)
        tag = f"max|dh|={a_dh:g} max|dc|={a_dc:g}"
        worst, runs = max(worst, (ratio, tag)), runs + 1
        ref = R.cell_backward_from_saved(gates.cpu(), cp.cpu(), c.cpu(), dh.cpu(), dc.cpu())
        w.close(res["dpre"], ref[0], 1e-5, f"dpre ({tag})")
        w.close(res["dcp"], ref[1], 1e-5, f"dc_prev ({tag})")
        assert res["dpre_amax"] == got
    _planes_line(f"lstm_pointwise_bwd bound attained c_bound={c_bound:g}", worst, runs)
    w.report()


def test_backward_planes_of_dead_samples_are_exact_zeros():
    """(B, P, C) = (3, 4, 256) with row_last: the dead samples' part of the operand decodes to exact zeros although their inputs hold NaN; the live
    samples' planes and dc_prev (and the scale pair) are bit-equal to the dense launch on zero-filled inputs"""
    from scanpaths_amd import functional as F
    B, P, C, step = 3, 4, 256, 2
    rows = B * P
    last = [0, 4, -1]
    dead, live = [0, 2], [1]
    state = _saved_state(B, P, C, seed=70)
    zs = _fill_samples(state, B, dead, 0.0)
    kw = dict(planes=True, dh_amax=_amax(zs[0]), dc_amax=_amax(zs[1]), c_bound=_amax(zs[4]), cprev_bound=_amax(zs[3]))
    dense = _bwd(*zs, **kw)
    sparse = _bwd(*_fill_samples(state, B, dead, NAN), last=torch.tensor(last, dtype=torch.int32, device=_dev()), step=step, rps=P, **kw)
    ratio, _ = _check_planes(sparse, rows, C)
    dec = _decode_split(F.SplitOperand(sparse["planes"], sparse["scale"], "f16x2"), (rows, 4 * C)).view(B, -1)
    assert float(dec[dead].abs().max()) == 0.0 and float(dec[live].abs().max()) > 0.0
    assert torch.equal(sparse["planes"], dense["planes"]) and torch.equal(sparse["scale"], dense["scale"])
    assert torch.equal(sparse["dcp"], dense["dcp"]) and torch.equal(sparse["dpre"], dense["dpre"])
    assert float(sparse["dcp"].view(B, -1)[dead].abs().max()) == 0.0
    _planes_line("lstm_pointwise_bwd planes row_last B=3 P=4 C=256", (ratio, "sparse launch"), 2)


# ====================================================================================================================
# 7: saturated gates
# ====================================================================================================================
def _tanh_small_argument(xg, gates, C):
    """worst relative error of the stored g gate over 0 < |pre| <= 1e-3 (pre = xg there: no hg, and the rank-1 term does not reach g), the
    number of such entries, and max|g| at pre = 0"""
    pre, g = xg.reshape(-1, 4 * C)[:, 3 * C:].double(), gates.reshape(-1, 4 * C)[:, 3 * C:].cpu().double()
    m = (pre.abs() <= float(torch.tensor(1e-3))) & (pre != 0)                      # (the float 1e-3 the inputs hold lies just above the double)
    assert int(m.sum()) > 0 and bool((pre == 0).any())
    return float(((g[m] - pre[m].tanh()).abs() / pre[m].tanh().abs()).max()), int(m.sum()), float(g[pre == 0].abs().max())


@pytest.mark.parametrize("kind,rows,C", [("pointwise", 3, 12), ("pointwise", 5, 64), ("rank1", 195, 64)])
def test_saturated_gates_stay_finite_and_within_the_stress_bar(kind, rows, C):
    """pre-activations from {+-100, +-88, +-20, +-1e-3, 0} among N(0, 1) entries, |c_prev| <= 17 (lstm_cell_ref.stress_inputs), through the
    pointwise forward, the rank-1 forward ((B, P) = (3, 65)) and the backward from the kernel's saved gates: every output finite, parity by
    max(bar, 10 max|ref32 - ref64|).  Records (no assertion) the worst relative error of the stored g gate for 0 < |pre| <= 1e-3, where the
    1 - 2 rcp(1 + exp2(.)) form of sp_tanh cancels."""
    w = Worst(f"saturation {kind} rows={rows} C={C}")
    xg, cp = R.stress_inputs(rows, C, seed=rows)
    dh, dc = R.randn(rows, C, seed=7), R.randn(rows, C, seed=8)
    sp = wc = None
    if kind == "rank1":
        B, P, KP = 3, 65, 20
        xg, cp = xg.view(B, P, 4 * C), cp.view(B, P, C)
        sp, wc = R.randn(B, P, KP, seed=9), R.randn(B, 3 * C, KP, seed=10, scale=0.2)
        rc, gates, c, h, hmax = _rank1_fwd(xg, None, cp, sp, wc)
        assert rc == 0 and hmax == _amax(h)
    else:
        gates, c, h = _fwd(xg, None, cp)
    r64, r32 = R.cell(xg, None, cp, sp, wc), R.cell(xg, None, cp, sp, wc, dtype=torch.float32)
    for got, k in ((gates, "gates"), (c, "c"), (h, "h")):
        assert bool(torch.isfinite(got).all()), k
        w.close(got, r64[k], stress_bar(3e-6, r32[k], r64[k]), k)
    g2, c2, cp2 = gates.view(rows, 4 * C), c.view(rows, C), cp.reshape(rows, C)
    res = _bwd(_d(dh), _d(dc), g2, _d(cp2), c2)
    b64 = R.cell_backward_from_saved(g2.cpu(), cp2, c2.cpu(), dh, dc)
    b32 = R.cell_backward_from_saved(g2.cpu(), cp2, c2.cpu(), dh, dc, dtype=torch.float32)
    for got, a, b, k in ((res["dpre"], b32[0], b64[0], "dpre"), (res["dcp"], b32[1], b64[1], "dc_prev")):
        assert bool(torch.isfinite(got).all()), k
        w.close(got, b, stress_bar(1e-5, a, b), k)
    assert res["dpre_amax"] == _amax(res["dpre"]) and res["dcp_amax"] == _amax(res["dcp"])
    rel, n, at0 = _tanh_small_argument(xg, gates, C)
    print(f"TANH {kind} rows={rows} C={C}: worst relative error of g = sp_tanh(pre) over 0 < |pre| <= 1e-3: {rel:.3e} ({n} entries), |g| at pre = 0: "
          f"{at0:.1e} (recorded, not asserted)")
    w.report()


# ====================================================================================================================
# 8: the cell as the epilogue of the h-gate conv
# ====================================================================================================================
FUSED_CASES = [(3, 4, 64, 20, 2, False),        # halo build, one tile per sample: both halo rows of every tile lie outside the image
               (3, 4, 64, 9, 1, False), (3, 4, 64, 32, 2, False), (3, 4, 64, 20, 2, True),
               (2, 2, 128, 20, 2, False), (2, 128, 2, 20, 2, False), (1, 1, 256, 20, 2, False), (1, 256, 1, 20, 2, False)]      # ordinary build


@pytest.mark.parametrize("B,Hm,Wm,KP,S,planes", FUSED_CASES)
def test_fused_cell_epilogue_at_one_tile_per_sample_and_extreme_aspect_ratios(B, Hm, Wm, KP, S, planes):
    """sp_gateconv_lstm_f16x2 through F.gateconv_lstm, C = 32, built like test_ops_gpu.test_lstm_cell_and_gate_conv and held to the same fp64 graph
    and bars, forward and every gradient.  FUSION_COUNTS shows the fused kernel ran (no silent fallback).  planes: with a bound on c_prev the
    epilogue also writes h's split operand -- the bound covers max|h| and the operand decodes to h within 2^-21 x bound."""
    from scanpaths_amd import functional as F
    from scanpaths_amd.notes import note, notes
    if F.SPLIT_SCHEME != "f16x2" or not F.USE_BF16X3:
        pytest.skip("2xfp16 back-end not active")
    C = 32
    assert 9 * S <= KP and (Hm * Wm) % 256 == 0
    w = Worst(f"gateconv_lstm B={B} {Hm}x{Wm} C={C} KP={KP} S={S} planes={planes}")
    h, c = _rand(B, C, Hm, Wm, seed=24), _rand(B, C, Hm, Wm, seed=25)
    xg = _rand(B, 4 * C, Hm, Wm, seed=26)
    wh = _rand(4 * C, C, 3, 3, seed=27, scale=0.1)
    sp = _rand(S, B, Hm, Wm, seed=28)
    wr = [_rand(3 * C, C, 3, 3, seed=29 + s, scale=0.1) for s in range(S)]
    se = _rand(S, B, C, seed=33)
    dbl = lambda t: t.double().requires_grad_(True)
    hr, cr, xgr, whr, spr, ser = dbl(h), dbl(c), dbl(xg), dbl(wh), dbl(sp), dbl(se)
    wrr = [dbl(t) for t in wr]
    pre = xgr + TF.conv2d(hr, whr, padding=1)
    extra = 0
    for s in range(S):
        ss = spr[s].unsqueeze(1) * ser[s].unsqueeze(-1).unsqueeze(-1)
        extra = extra + TF.conv2d(ss, wrr[s], padding=1)
    pre = pre + torch.cat([extra, torch.zeros_like(extra[:, :C])], 1)
    i, f, o, g = pre[:, :C].sigmoid(), pre[:, C:2 * C].sigmoid(), pre[:, 2 * C:3 * C].sigmoid(), pre[:, 3 * C:].tanh()
    c2 = f * cr + i * g
    h2 = o * c2
    gh, gc = _rand(*h2.shape, seed=40), _rand(*c2.shape, seed=41)
    (h2 * gh.double()).sum().add((c2 * gc.double()).sum()).backward()

    dev = _dev()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dev).requires_grad_(True)
    hg_, cg_, xgg = nhwc(h), nhwc(c), nhwc(xg)
    whg = wh.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
    spg, seg = sp.to(dev).requires_grad_(True), se.to(dev).requires_grad_(True)
    wrg = [t.to(dev).contiguous(memory_format=torch.channels_last).requires_grad_(True) for t in wr]
    parts = []
    for s in range(S):
        wflat = wrg[s].permute(0, 2, 3, 1).reshape(3 * C * 9, C)
        parts.append(F.gemm(seg[s], wflat, None, "nk").view(B, 3 * C, 9))
    wc = torch.cat(parts + [torch.zeros(B, 3 * C, KP - 9 * S, device=dev)], 2)
    spcol = F.im2col3x3(spg, KP)
    if planes:
        note(cg_).cbound = math.ceil(float(c.abs().max())) + 0.5          # (exact as a float, and so is the bound + 1 the kernel receives)
    F.reset_fusion_counts()
    hn, cn = F.gateconv_lstm(hg_, whg, xgg, cg_, spcol, wc, {})
    assert F.FUSION_COUNTS["gateconv_lstm"] == 1
    if planes:
        assert F.FUSION_COUNTS["gateconv_lstm_hplanes"] == 1
        op = notes(hn).cache["f16x2"]
        bound = float(op.scale[1])
        assert bound == notes(cg_).cbound + 1.0 and float(hn.detach().abs().max()) <= bound
        derr = float((_decode_split(op, hn.shape) - hn.detach()).abs().max())
        assert derr <= 2.0 ** -21 * bound, (derr, bound)
    else:
        assert float(notes(hn).amax[1]) == float(hn.detach().abs().max())          # fused max|h| hint (float bits in slot 1)
    (hn * nhwc(gh).detach()).sum().add((cn * nhwc(gc).detach()).sum()).backward()
    back = lambda t: t.permute(0, 3, 1, 2)
    w.close(back(hn), h2, 3e-6, "h")
    w.close(back(cn), c2, 3e-6, "c")
    w.close(back(hg_.grad), hr.grad, 1e-5, "dh")
    w.close(back(cg_.grad), cr.grad, 1e-5, "dc")
    w.close(back(xgg.grad), xgr.grad, 1e-5, "dxg")
    w.close(whg.grad, whr.grad, 1e-5, "dwh")
    w.close(spg.grad, spr.grad, 1e-5, "dspatial")
    w.close(seg.grad, ser.grad, 1e-5, "dsemantic")
    for s in range(S):
        w.close(wrg[s].grad, wrr[s].grad, 1e-5, f"dwr{s}")
    w.report()
