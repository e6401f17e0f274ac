"""tests/rank1_grads_ref.py against torch.bmm in fp64 and against its own claims: the teeth of the element-wise bars (one pixel, one group of 16
channels) and the exactness condition of the lattice cases.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import f16x2_ref as X
import parity as P
import rank1_grads_ref as R

CASES = R.cases()


@functools.lru_cache(maxsize=None)
def problem(case):
    return R.Problem(case)


def test_case_list_covers_the_axes():
    cs = R.pairwise_cases()
    assert 20 <= len(cs) <= 32, len(cs)
    for axis, values in (("KP", R.KPS), ("P", R.PS), ("N3", R.N3S), ("B", R.BS), ("dead", R.DEADS), ("kind", R.KINDS)):
        assert {getattr(c, axis) for c in cs} == set(values), axis
    assert {c.ldy - c.N3 for c in cs} >= {0, 16} and any(c.ldy * 3 == c.N3 * 4 for c in cs)
    assert [len(range(0, min(R.CHUNK, c - o), 32)) for c in (352,) for o in (0, 160, 320)] == [5, 5, 1]
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)


def test_tap_scale_is_the_kernels():
    assert R.tap_scale(0.0) == np.float32(2.0 ** 127)                          # e = 0: clamped at 254
    assert R.tap_scale(1.0) == np.float32(2.0 ** 14) and R.tap_scale(1.99) == np.float32(2.0 ** 14) and R.tap_scale(2.0) == np.float32(2.0 ** 13)
    assert R.tap_scale(2.0 ** -120) == np.float32(2.0 ** 127)                  # 134 would be needed
    assert R.tap_scale(2.0 ** -113) == np.float32(2.0 ** 127) and R.tap_scale(2.0 ** -112) == np.float32(2.0 ** 126)
    assert R.tap_scale(2.0 ** 100) == np.float32(2.0 ** -86)
    assert R.tap_scale(3.0e38) == np.float32(2.0 ** -113)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_contractions_match_torch_bmm(case):
    p, c = problem(case), case
    y1, y2 = X.unpack(p.Yp, c.B * c.P, c.N3, c.ldy)
    w1, w2 = X.unpack(p.Wp, c.B * c.KP, c.N3)
    t = lambda a, *shape: torch.from_numpy(a).reshape(*shape)
    y1, y2 = t(y1, c.B, c.P, c.N3), t(y2, c.B, c.P, c.N3)
    w1, w2 = t(w1, c.B, c.KP, c.N3).transpose(1, 2), t(w2, c.B, c.KP, c.N3).transpose(1, 2)
    sw = torch.from_numpy(p.sw.astype(np.float64)).reshape(c.B, 1, c.KP)
    want = (torch.bmm(y1, w1) + torch.bmm(y1, w2) + torch.bmm(y2, w1)) / float(p.sy) / sw
    ref, S = p.dsp_planes()
    assert ((ref - want).abs() <= 1e-12 * S + 1e-300).all()
    assert ((p.dsp_true() - torch.bmm(torch.from_numpy(p.dpre).double(), torch.from_numpy(p.wcT).double().transpose(1, 2))).abs() <= 1e-12 * S + 1e-300).all()
    # dwc: the taps split per (sample, chunk) by an independent loop
    want = torch.zeros(c.B, c.N3, c.KP, dtype=torch.float64)
    for b in range(c.B):
        for ch in range(p.chunks):
            px = slice(ch * 160, min(c.P, ch * 160 + 160))
            tp = p.taps[b, px]
            m = np.float32(np.abs(tp).max())
            s = np.float32(2.0) ** min(127, max(-126, 14 - (int(np.frexp(m)[1]) - 1))) if m > 0 else np.float32(2.0 ** 127)
            assert s == p.st[b, ch], (b, ch, s, p.st[b, ch])
            xs = (tp * s).astype(np.float32)
            th = xs.astype(np.float16)
            tl = (xs - th.astype(np.float32)).astype(np.float16)
            th, tl = torch.from_numpy(th.astype(np.float64)), torch.from_numpy(tl.astype(np.float64))
            a1, a2 = y1[b, px].T, y2[b, px].T
            want[b] += (a2 @ th + a1 @ tl + a1 @ th) / float(s) / float(p.sy)
    ref, S = p.dwc_planes()
    assert ((ref - want).abs() <= 1e-12 * S + 1e-300).all()
    assert ((p.dwc_true() - torch.bmm(torch.from_numpy(p.dpre).double().transpose(1, 2), torch.from_numpy(p.taps).double())).abs()
            <= 1e-12 * p.dwc_true().abs().max() + 1e-300).all()
    # the planes stand for the fp32 operands within the derived representation bound
    assert ((p.dsp_planes()[0] - p.dsp_true()).abs() <= p.dsp_rep()).all()
    assert ((p.dwc_planes()[0] - p.dwc_true()).abs() <= p.dwc_rep()).all()


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_bars_have_teeth(case):
    """leaving out one group of 16 channels (dsp) or one pixel (dwc) moves some element by more than its bar"""
    p, c = problem(case), case
    ref, S = p.dsp_planes()
    less, _ = p.dsp_planes(drop_group=c.N3 // 16 - 1)
    assert ((ref - less).abs() > P.bar(S, p.chain_dsp)).any(), "dsp"
    if c.kind == "zero-all":                # every tap is zero: dwc is zero whatever is left out (the GPU test asserts the exact zeros)
        assert not p.dwc_planes()[0].any()
        return
    ref, S = p.dwc_planes()
    less, _ = p.dwc_planes(drop_pixel=p.teeth_pixel())
    assert ((ref - less).abs() > P.bar(S, p.chain_dwc)).any(), "dwc"


@pytest.mark.parametrize("case", [c for c in CASES if c.kind == "lattice"], ids=lambda c: c.name)
def test_lattice_cases_are_exact_in_every_order(case):
    p = problem(case)
    for v, planes in ((p.taps, (p.T1, p.T2)),):
        assert torch.equal((planes[0] + planes[1]) / torch.from_numpy(np.repeat(p.st, 160, axis=1)[:, :case.P, None].astype(np.float64)),
                           torch.from_numpy(v.astype(np.float64))), "the tap planes are not exact"
    assert torch.equal((p.Y1 + p.Y2) / float(p.sy), torch.from_numpy(p.dpre.astype(np.float64)))
    dsp, dwc = p.exact_spans()
    assert dsp <= 2.0 ** 24 and dwc <= 2.0 ** 24, (dsp, dwc)


def test_chains():
    assert R.chain_dsp(256) == X._chain(2 * 96 * 8 + 2) and R.chain_dsp(768) == X._chain(2 * 96 * 24 + 2)
    assert R.chain_dwc(32) == X._chain(2 * 96 * 1 + 2 + 1) and R.chain_dwc(352) == X._chain(2 * 96 * 5 + 6 + 1)
    assert R.chain_dwc(128) == X._chain(2 * 96 * 4 + 3)
