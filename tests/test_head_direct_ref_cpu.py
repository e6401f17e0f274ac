"""tests/head_direct_ref.py against torch in fp64 -- the literal two-conv formulation of predict_head that
test_direct_head_matches_two_conv_formulation uses (a 5 x 5 conv with the composed filters, then the one-hot 7 x 7 stride-5 pad-2 tap sum over the
zero-padded intermediate map) and torch autograd for every gradient -- at 1e-12, on every map of the GPU case list; and against its own claims: the
site table of the issue, the chains, the teeth of the element-wise bars, the exactness condition of the lattice cases.  No GPU."""
import functools

import pytest
import torch
import torch.nn.functional as TF

import parity as P
import head_direct_ref as R

CASES = R.cases()


@functools.lru_cache(maxsize=None)
def problem(case, kind="gauss"):
    return R.Problem(case, kind)


def _same(a, b, scale=None):
    scale = float(b.abs().max()) if scale is None else scale
    return float((a - b).abs().max()) <= 1e-12 * max(scale, 1e-300)


def test_site_table():
    for side, (n, ncls) in R.SIDES.items():
        a = R.axis(side)
        assert (a.n, len(a.masks)) == (n, ncls), side
        assert a.n == (side - 3) // 5 + 1
    assert R.axis(1) is None and R.axis(2) is None and R.axis(163) is None and R.axis(162).n == 32
    assert R.num_classes(2, 40) == -1 and R.num_classes(40, 163) == -1 and R.num_classes(40, 64) == 6 and R.num_classes(13, 38) == 9
    assert R.axis(3).masks == [(False, False, True, True, True, False, False)]          # clipped on both sides
    assert R.axis(15).cls == [0, 1, 1]                                                  # the last class equals the interior
    assert R.Geo(23, 133).S == 135 and R.Geo(38, 8).ay.n == 8 and R.Geo(8, 40).ax.n == 8


def test_case_list_covers_the_axes():
    assert 28 <= len(CASES) <= 34
    assert {(c.Hm, c.Wm) for c in CASES} == {(3, 3), (7, 8), (13, 15), (38, 8), (40, 13), (8, 40), (23, 133), (3, 162), (162, 3)}
    assert {c.B for c in CASES} == {1, 3, 4, 5, 9} and {c.C for c in CASES} == {4, 12, 516} and {c.nsel for c in CASES} == {1, 2, 3, 9}
    assert {c.nheads for c in CASES} == {1, 2, 3} and {c.HC for c in CASES} == {64, 51} and {c.hmap for c in CASES} == {"same", "mixed", "unused"}
    assert {c.B for c in CASES if (c.Hm, c.Wm) in ((38, 8), (40, 13))} >= {4, 5}
    for c in CASES:
        m = R.make_hmap(c)
        if c.hmap == "same":
            assert (m == m[0]).all()
        if c.hmap == "mixed":
            assert (m[:min(4, c.B)] != m[0]).any(), c.name
        if c.hmap == "unused":
            assert int(m.max()) < c.nheads - 1 and c.nheads > 1, c.name
        assert all(side in R.SIDES for side in (c.Hm, c.Wm))


def _two_conv(p, h, Gf, cb):
    """[B, nheads, HC, Hm, Wm] and Dpre [nsel, B, S] by the literal formulation (torch, differentiable)"""
    c, geo = p.c, p.geo
    Z = TF.conv2d(h.reshape(c.B, c.Hm, c.Wm, c.C).permute(0, 3, 1, 2), Gf.reshape(c.nheads * c.HC, 5, 5, c.C).permute(0, 3, 1, 2), None, padding=2)
    Z = Z.view(c.B, c.nheads, c.HC, c.Hm, c.Wm)
    eye = torch.eye(49, dtype=torch.float64).view(1, 49, 7, 7)
    D = []
    for i in range(c.nsel):
        row = []
        for b in range(c.B):
            k = int(p.hmap[b, i])
            inter = Z[b, k, 2:51] + cb[k, 2:51].view(49, 1, 1)
            row.append(TF.conv2d(inter.unsqueeze(0), eye, None, stride=5, padding=2).reshape(geo.S))
        D.append(torch.stack(row))
    return Z, torch.stack(D)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_duration_sites_match_the_two_conv_formulation(case):
    p, c, geo = problem(case), case, problem(case).geo
    h, Gf, cb = (t.double().requires_grad_(True) for t in (p.h, p.G, p.cb))
    Z, D_t = _two_conv(p, h, Gf, cb)
    (W11, cbsum), _ = R.compose11_fwd(p.G, p.cb, geo)
    D, S = R.drt_fwd(p.h, W11, cbsum, p.hmap, geo, c.nsel)
    assert _same(D, D_t.detach(), float(S.max()))
    (D_t * p.dD.double()).sum().backward()
    dh, S = R.drt_bwd_data(p.dD, W11, p.hmap, geo, c.nsel)
    assert _same(dh, h.grad, float(S.max()))
    (dW11, dcbsum), _ = R.drt_bwd_weight(p.dD, p.h, p.hmap, geo, c.nsel, c.nheads)
    (dG, dcb), (SG, Scb) = R.compose11_bwd(dW11, dcbsum, geo, c.HC)
    assert _same(dG, Gf.grad, float(SG.max())) and _same(dcb, cb.grad, float(Scb.max()))
    assert not dG[:, :2].any() and not dG[:, 51:].any() and not dcb[:, :2].any() and not dcb[:, 51:].any()
    if c.hmap == "unused":
        assert not dW11[c.nheads - 1].any() and not dcbsum[c.nheads - 1].any()
    # accumulate
    dh1, _ = R.drt_bwd_data(p.dD, W11, p.hmap, geo, c.nsel, dh0=p.dh0)
    assert torch.equal(dh1, dh + p.dh0.double())


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_saliency_gather_matches_the_conv_and_autograd(case):
    p, c, geo = problem(case), case, problem(case).geo
    Z, _ = _two_conv(p, p.h.double(), p.G.double(), p.cb.double())
    nsrc = c.nheads
    for ldt in (50 * nsrc, 50 * nsrc + 14):
        # the tap partials: the 1 x 1 GEMM of h with G's rows 0 / 1 reshaped [(src 2 + o) 25 + tap][C]
        T = torch.zeros(c.B, geo.P, ldt, dtype=torch.float64)
        T[:, :, :50 * nsrc] = torch.einsum("bqc,kouc->bqkou", p.h.double(), p.G.double()[:, :2].reshape(nsrc, 2, 25, c.C)).reshape(c.B, geo.P, -1)
        T.requires_grad_(True)
        Z2, S = R.sal_gather_fwd(T.detach(), p.hmap, c.Hm, c.Wm, c.nsel)
        want = torch.stack([torch.stack([Z[b, int(p.hmap[b, j >> 1]), j & 1].reshape(geo.P) for j in range(c.nsel * 2)], -1) for b in range(c.B)])
        assert _same(Z2, want, float(S.max()))
        # torch's own gather (pad, shifted slices) for the adjoint
        Tp = TF.pad(T.view(c.B, c.Hm, c.Wm, ldt), (0, 0, 2, 2, 2, 2))
        cols = []
        for b in range(c.B):
            for j in range(c.nsel * 2):
                col0 = (int(p.hmap[b, j >> 1]) * 2 + (j & 1)) * 25
                cols.append(sum(Tp[b, uy:uy + c.Hm, ux:ux + c.Wm, col0 + uy * 5 + ux] for uy in range(5) for ux in range(5)))
        Zt = torch.stack(cols).view(c.B, c.nsel * 2, geo.P).transpose(1, 2)
        assert _same(Zt.detach(), Z2, float(S.max()))
        dZ2 = p.dZ2().double()
        (Zt * dZ2).sum().backward()
        dT, S = R.sal_gather_bwd(dZ2, p.hmap, c.Hm, c.Wm, c.nsel, nsrc, ldt)
        assert _same(dT, T.grad, float(S.max())) and not dT[:, :, 50 * nsrc:].any()
    dead = [0] if c.B == 1 else [1, c.B - 1]
    dZn = dZ2.clone()
    dZn[dead] = float("nan")
    dTd, _ = R.sal_gather_bwd(dZn, p.hmap, c.Hm, c.Wm, c.nsel, nsrc, ldt, dead=dead)
    live = [b for b in range(c.B) if b not in dead]
    assert not dTd[dead].any() and torch.equal(dTd[live], dT[live])


def test_flags_only_leave_out_exact_zeros():
    c = R.cases()[4]
    p, geo = problem(c), problem(c).geo
    live = torch.ones(c.nsel, c.B, dtype=torch.int32)
    live[1, 0] = live[0, 2] = 0                     # (row 0 is dead by row_last as well)
    on = R.dead_pairs(c.B, c.nsel, live, [0, 5, 9, 9, 0], 5)
    assert on.tolist() == [[False, True, False, True, False], [False, True, True, True, False]]
    assert R.dead_pairs(6, 1, None, [0, 1, 5], 1, 3).tolist() == [[False, True, True, False, False, True]]
    dD = p.dD.clone()
    dD[~on] = 0
    for f in (lambda **kw: R.drt_bwd_data(dD, p.W11, p.hmap, geo, c.nsel, **kw)[0],
              lambda **kw: R.drt_bwd_weight(dD, p.h, p.hmap, geo, c.nsel, c.nheads, **kw)[0][0]):
        assert torch.equal(f(on=on), f())


def _entries(p):
    """(name, ref and S with nothing left out, the same with one term left out, chain, lattice unit) of every kernel on the case's own operands"""
    c, geo, nsrc = p.c, p.geo, p.c.nheads
    T, dZ2 = p.T(nsrc, 50 * nsrc), p.dZ2()
    rows = []
    (W, cs), (SW, Scs) = R.compose11_fwd(p.G, p.cb, geo)
    (Wd, csd), _ = R.compose11_fwd(p.G, p.cb, geo, drop=True)
    rows += [("compose_fwd", W, SW, Wd, R.chain_compose11_fwd(), p.unit["compose_fwd"]),
             ("compose_fwd_cb", cs, Scs, csd, R.chain_compose11_fwd(), p.unit["compose_fwd_cb"])]
    (dG, dcb), (SG, Scb) = R.compose11_bwd(p.dW11, p.dcbsum, geo, c.HC)
    (dGd, dcbd), _ = R.compose11_bwd(p.dW11, p.dcbsum, geo, c.HC, drop=True)
    rows += [("compose_bwd", dG, SG, dGd, R.chain_compose11_bwd(geo.ncls), p.unit["compose_bwd"]),
             ("compose_bwd_cb", dcb, Scb, dcbd, R.chain_dcbsum(), p.unit["compose_bwd_cb"])]
    Z2, S = R.sal_gather_fwd(T, p.hmap, c.Hm, c.Wm, c.nsel)
    rows.append(("gather_fwd", Z2, S, R.sal_gather_fwd(T, p.hmap, c.Hm, c.Wm, c.nsel, drop=True)[0], R.chain_sal_gather_fwd(), p.unit["gather"]))
    dT, S = R.sal_gather_bwd(dZ2, p.hmap, c.Hm, c.Wm, c.nsel, nsrc, 50 * nsrc)
    rows.append(("gather_bwd", dT, S, R.sal_gather_bwd(dZ2, p.hmap, c.Hm, c.Wm, c.nsel, nsrc, 50 * nsrc, drop=True)[0],
                 R.chain_sal_gather_bwd(c.nsel), p.unit["gather"]))
    D, S = R.drt_fwd(p.h, p.W11, p.cbsum, p.hmap, geo, c.nsel)
    rows.append(("drt_fwd", D, S, R.drt_fwd(p.h, p.W11, p.cbsum, p.hmap, geo, c.nsel, drop=True)[0], R.chain_drt_fwd(geo, c.C), p.unit["drt_fwd"]))
    for acc in (0, 1):
        dh0 = p.dh0 if acc else None
        dh, S = R.drt_bwd_data(p.dD, p.W11, p.hmap, geo, c.nsel, dh0=dh0)
        rows.append((f"bwd_data_acc{acc}", dh, S, R.drt_bwd_data(p.dD, p.W11, p.hmap, geo, c.nsel, dh0=dh0, drop=True)[0],
                     R.chain_drt_bwd_data(c.nsel, acc), p.unit["bwd_data"]))
    (dW, dcs), (SW, Scs) = R.drt_bwd_weight(p.dD, p.h, p.hmap, geo, c.nsel, c.nheads)
    for drop in ("slab", "site"):
        (dWd, dcsd), _ = R.drt_bwd_weight(p.dD, p.h, p.hmap, geo, c.nsel, c.nheads, drop=drop)
        rows += [(f"bwd_weight_drop_{drop}", dW, SW, dWd, R.chain_drt_bwd_weight(geo, p.hmap, c.nheads), p.unit["bwd_weight"]),
                 (f"dcbsum_drop_{drop}", dcs, Scs, dcsd, R.chain_dcbsum(), p.unit["dcbsum"])]
    return rows


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_bars_have_teeth(case):
    """one term left out -- the last in-map tap of a window, one site, one (b, i) slab, one class, one slot -- moves some element by more than its bar"""
    for name, ref, S, less, chain, _ in _entries(problem(case)):
        assert ((ref - less).abs() > P.bar(S, chain)).any(), name


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_lattice_cases_are_exact_in_every_order(case):
    for name, ref, S, _, _, unit in _entries(problem(case, "lattice")):
        assert float(S.max()) / unit <= 2.0 ** 24, (name, float(S.max()) / unit)
        assert torch.equal(ref, (ref / unit).round() * unit) and torch.equal(ref, ref.float().double()), name


def test_chains():
    g = R.Geo(40, 64)
    assert g.max_taps() == 121 and R.chain_drt_fwd(g, 32) == 4 * 4 + 11 and R.chain_drt_fwd(R.Geo(3, 3), 516) == 4 * 5 + 11
    assert R.chain_drt_bwd_data(2, 1) == 38 and R.chain_compose11_fwd() == 50 and R.chain_sal_gather_fwd() == 26
    assert g.max_class_sites() == 7 * 11 and R.chain_drt_bwd_weight(g, torch.tensor([[0, 1]] * 3), 2) == 2 * 77 + 3 + 1
