"""The entry points of csrc/head_direct.hip through the C ABI -- sp_head_num_classes, sp_head_compose11_fwd / bwd, sp_sal_gather_fwd / bwd,
sp_drt_direct_fwd, sp_drt_direct_bwd_data, sp_drt_direct_bwd_weight and its workspace query -- against the plain fp64 restatement of
tests/head_direct_ref.py (held to torch's fp64 conv and autograd by tests/test_head_direct_ref_cpu.py), at the shapes where the kernels change
path: full groups of four rows and group boundaries, the XCD site order, odd and > 8 slot counts, the second compaction round (S = 135), C / 4 > 128,
one-site axes clipped on both sides, the 32-site limit, heads that no row selects, accumulate, padded ldt, dead rows.

Float operands lie between NaN guards, outputs and the workspace (exactly the queried size) between sentinel guards (parity.Guarded): after each
launch every word outside the live region is unchanged and every live word finite and inside the ELEMENT-WISE bar parity.bar(S, chain) (chains:
head_direct_ref.chain_*).  The max-norm bars tests/test_ops_gpu.py holds these ops to (2e-5 forward, 3e-5 gradients) stay as a second assertion.
Every case runs on Gaussian data and on lattice data (small integers times a power of two: every summation order is exact), where the kernel must
equal the fp64 result exactly (torch.equal in fp64).  sp_drt_direct_fwd and sp_drt_direct_bwd_weight run twice and must be bit-identical.  Each
comparison prints a PARITY line, the module a summary per group (profiles/head_direct_parity.md)."""
import functools

import pytest
import torch

import head_direct_ref as R
import parity as P

pytestmark = pytest.mark.gpu

EINVAL, ENULL = -1, -2
GROUPS = ("head_compose11_fwd", "head_compose11_bwd", "head_compose11_dcb", "head_sal_gather_fwd", "head_sal_gather_bwd", "head_drt_fwd", "head_drt_bwd_data",
          "head_drt_bwd_weight", "head_drt_dcbsum")
FWD, GRAD = 2e-5, 3e-5            # the max-norm bars of test_direct_head_matches_two_conv_formulation


SUM = P.Summary("head_direct", GROUPS)
_summary = SUM.fixture()
_problem = functools.lru_cache(maxsize=None)(R.Problem)          # (case, kind) -> operands and restatement, built once


def _p(t):
    return None if t is None else t.data_ptr()


def _check(group, name, out, ref, S, chain, legacy, lattice):
    SUM.judge(group, name, out.g, out.flat(), ref.reshape(1, 1, -1), S.reshape(1, 1, -1), chain, legacy)
    if lattice:
        SUM.exact(group, name, out.live(), ref)


def _sync(rc, what):
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)


# ====================================================================================================================
# launches
# ====================================================================================================================
def _drt_fwd(p, h, W11, cbsum):
    hip, L = P.abi()
    c = p.c
    out = P.output(c.nsel * c.B * p.geo.S)
    a, w, cs, hm = P.operand(h), P.operand(W11), P.operand(cbsum), P.ints(p.hmap)
    _sync(L.sp_drt_direct_fwd(a.ptr, w.ptr, cs.ptr, _p(hm), c.B, c.Hm, c.Wm, c.C, c.nsel, out.ptr, hip.stream()), "sp_drt_direct_fwd")
    return out


def _bwd_data(p, dD, W11, accumulate, dh0, live=None, row_last=None, row_step=0, rowB=0):
    hip, L = P.abi()
    c, B = p.c, p.c.B
    out = P.output(B * p.geo.P * c.C, dh0)
    g, w, hm, lv, rl = P.operand(dD), P.operand(W11), P.ints(p.hmap), P.ints(live), P.ints(row_last)
    _sync(L.sp_drt_direct_bwd_data(g.ptr, w.ptr, _p(hm), B, c.Hm, c.Wm, c.C, c.nsel, accumulate, out.ptr, _p(lv), _p(rl), row_step, rowB, hip.stream()),
          "sp_drt_direct_bwd_data")
    return out


def _bwd_weight(p, dD, h, live=None, row_last=None, row_step=0, rowB=0):
    """-> (dW11, dcbsum, workspace)"""
    hip, L = P.abi()
    c, B = p.c, p.c.B
    nbytes = L.sp_drt_direct_bwd_weight_workspace(B, c.Hm, c.Wm, c.C, c.nsel)
    assert nbytes == B * c.nsel * p.geo.ncls * 121 * c.C * 4, nbytes
    ws, dW, dcs = P.output(nbytes // 4), P.output(c.nheads * p.geo.ncls * 121 * c.C), P.output(c.nheads * p.geo.ncls)
    g, a, hm, lv, rl = P.operand(dD), P.operand(h), P.ints(p.hmap), P.ints(live), P.ints(row_last)
    _sync(L.sp_drt_direct_bwd_weight(g.ptr, a.ptr, _p(hm), B, c.Hm, c.Wm, c.C, c.nsel, c.nheads, ws.ptr, dW.ptr, dcs.ptr, _p(lv), _p(rl), row_step, rowB,
                                     hip.stream()), "sp_drt_direct_bwd_weight")
    assert ws.pads_untouched(), "a word around the slab workspace changed"
    return dW, dcs, ws


def _gather_bwd(p, dZ2, nsrc, ldt, row_last=None, row_step=0):
    hip, L = P.abi()
    c = p.c
    out = P.output(c.B * p.geo.P * ldt)
    g, hm, rl = P.operand(dZ2), P.ints(p.hmap), P.ints(row_last)
    _sync(L.sp_sal_gather_bwd(g.ptr, c.B, c.Hm, c.Wm, ldt, c.nsel, nsrc, _p(hm), out.ptr, _p(rl), row_step, hip.stream()), "sp_sal_gather_bwd")
    return out


# ====================================================================================================================
# parity
# ====================================================================================================================
def _cases(f):
    """every case on both kinds of data; the test gets (problem, case, geometry, lattice?, name)"""
    @pytest.mark.parametrize("kind", ["gauss", "lattice"])
    @pytest.mark.parametrize("case", R.cases(), ids=lambda c: c.name)
    def test(case, kind):
        p = _problem(case, kind)
        f(p, case, p.geo, kind == "lattice", f"{case.name}-{kind}")
    test.__name__, test.__doc__ = f.__name__, f.__doc__
    return test


@_cases
def test_compose11(p, c, geo, lat, name):
    hip, L = P.abi()
    assert L.sp_head_num_classes(c.Hm, c.Wm) == geo.ncls
    (W, cs), (SW, Scs) = R.compose11_fwd(p.G, p.cb, geo)
    a, b, oW, ocs = P.operand(p.G), P.operand(p.cb), P.output(W.numel()), P.output(cs.numel())
    _sync(L.sp_head_compose11_fwd(a.ptr, b.ptr, c.nheads, c.HC, c.C, c.Hm, c.Wm, oW.ptr, ocs.ptr, hip.stream()), "sp_head_compose11_fwd")
    _check("head_compose11_fwd", name + "-W11", oW, W, SW, R.chain_compose11_fwd(), FWD, lat)
    _check("head_compose11_fwd", name + "-cbsum", ocs, cs, Scs, R.chain_compose11_fwd(), FWD, lat)
    (dG, dcb), (SG, Scb) = R.compose11_bwd(p.dW11, p.dcbsum, geo, c.HC)
    a, b, oG, ocb = P.operand(p.dW11), P.operand(p.dcbsum), P.output(dG.numel()), P.output(dcb.numel())
    _sync(L.sp_head_compose11_bwd(a.ptr, b.ptr, c.nheads, c.HC, c.C, c.Hm, c.Wm, oG.ptr, ocb.ptr, hip.stream()), "sp_head_compose11_bwd")
    _check("head_compose11_bwd", name + "-dG", oG, dG, SG, R.chain_compose11_bwd(geo.ncls), GRAD, lat)
    _check("head_compose11_dcb", name, ocb, dcb, Scb, R.chain_dcbsum(), GRAD, lat)          # an fp64 sum rounded once


@_cases
def test_sal_gather(p, c, geo, lat, name):
    """ldt = 50 nsrc and 50 nsrc + 14: NaN in the pad columns of T (not read), zeros required in those of dT"""
    hip, L = P.abi()
    nsrc, hm = c.nheads, P.ints(p.hmap)
    dZ2 = p.dZ2()
    for ldt in (50 * nsrc, 50 * nsrc + 14):
        T = p.T(nsrc, ldt)
        Z2, S = R.sal_gather_fwd(T, p.hmap, c.Hm, c.Wm, c.nsel)
        Tn = T.clone()
        Tn[:, :, 50 * nsrc:] = float("nan")
        a, oZ = P.operand(Tn), P.output(Z2.numel())
        _sync(L.sp_sal_gather_fwd(a.ptr, c.B, c.Hm, c.Wm, ldt, c.nsel, _p(hm), oZ.ptr, hip.stream()), "sp_sal_gather_fwd")
        _check("head_sal_gather_fwd", f"{name}-ldt{ldt}", oZ, Z2, S, R.chain_sal_gather_fwd(), FWD, lat)
        dT, S = R.sal_gather_bwd(dZ2, p.hmap, c.Hm, c.Wm, c.nsel, nsrc, ldt)
        oT = _gather_bwd(p, dZ2, nsrc, ldt)
        _check("head_sal_gather_bwd", f"{name}-ldt{ldt}", oT, dT, S, R.chain_sal_gather_bwd(c.nsel), GRAD, lat)
        assert not oT.live().reshape(c.B, geo.P, ldt)[:, :, 50 * nsrc:].any(), f"{name}: the pad columns of dT are not zeros"


@_cases
def test_drt_fwd(p, c, geo, lat, name):
    D, S = R.drt_fwd(p.h, p.W11, p.cbsum, p.hmap, geo, c.nsel)
    oD = _drt_fwd(p, p.h, p.W11, p.cbsum)
    _check("head_drt_fwd", name, oD, D, S, R.chain_drt_fwd(geo, c.C), FWD, lat)
    assert P.same_bits(oD.flat(), _drt_fwd(p, p.h, p.W11, p.cbsum).flat()), f"{name}: two sp_drt_direct_fwd launches differ"


@_cases
def test_drt_bwd_data(p, c, geo, lat, name):
    for acc in (0, 1):
        dh0 = p.dh0 if acc else None
        dh, S = R.drt_bwd_data(p.dD, p.W11, p.hmap, geo, c.nsel, dh0=dh0)
        _check("head_drt_bwd_data", f"{name}-accumulate{acc}", _bwd_data(p, p.dD, p.W11, acc, dh0), dh, S, R.chain_drt_bwd_data(c.nsel, acc), GRAD, lat)


@_cases
def test_drt_bwd_weight(p, c, geo, lat, name):
    (dW, dcs), (SW, Scs) = R.drt_bwd_weight(p.dD, p.h, p.hmap, geo, c.nsel, c.nheads)
    oW, ocs, ws = _bwd_weight(p, p.dD, p.h)
    assert torch.isfinite(ws.live()).all(), f"{name}: a slab of a live pair was not written"
    _check("head_drt_bwd_weight", name, oW, dW, SW, R.chain_drt_bwd_weight(geo, p.hmap, c.nheads), GRAD, lat)
    _check("head_drt_dcbsum", name, ocs, dcs, Scs, R.chain_dcbsum(), GRAD, lat)
    oW2, ocs2, _ = _bwd_weight(p, p.dD, p.h)
    assert P.same_bits(oW.flat(), oW2.flat()) and P.same_bits(ocs.flat(), ocs2.flat()), f"{name}: two sp_drt_direct_bwd_weight launches differ"
    if c.hmap == "unused":
        k = c.nheads - 1
        assert not oW.live().reshape(c.nheads, -1)[k].any() and not ocs.live().reshape(c.nheads, -1)[k].any(), f"{name}: a head no row selects"


# ====================================================================================================================
# the zero-gradient contract
# ====================================================================================================================
_Z = R.Case
ZERO = [  # (name, case, rowB, row_last, row_step, [(slot, row)] switched off in `live`); a row with row_last == its step is alive
    ("per-step", _Z("zero-13x15", 13, 15, 5, 12, 2, 2, 64, "mixed"), 5, [0, 5, 9, 2, 9], 5, [(1, 1), (0, 2)]),
    ("two-steps-straddling-a-group", _Z("zero-38x8", 38, 8, 6, 4, 3, 3, 64, "mixed"), 3, [0, 1, 5], 1, [(2, 2)]),
    ("nsel9-flags-ignored", _Z("zero-7x8", 7, 8, 4, 4, 9, 2, 64, "same"), 4, [9, 0, 3, 9], 3, [(0, 0), (3, 2), (8, 3)]),      # slot 8 of row 0 is alive where slot 0 is not
]


@pytest.mark.parametrize("name,case,rowB,row_last,row_step,off", ZERO, ids=[z[0] for z in ZERO])
def test_zero_gradient_contract(name, case, rowB, row_last, row_step, off):
    """dead (row, slot) pairs hold exact zeros in dDpre and NaN in h: the flagged launches are finite and equal, bit for bit, the launches without
    flags on the same dDpre with finite h; dh of dead rows is zero (accumulate = 0) or keeps its value (accumulate = 1)"""
    p, c, geo = _problem(case, "gauss"), case, _problem(case, "gauss").geo
    live = torch.ones(c.nsel, c.B, dtype=torch.int32)
    for i, b in off:
        live[i, b] = 0
    on = R.dead_pairs(c.B, c.nsel, live, row_last, row_step, rowB)
    dead_rows = [b for b in range(c.B) if not on[:, b].any()]
    assert dead_rows and any(0 < int(on[:, b].sum()) < c.nsel for b in range(c.B)), "the case has dead rows and half-dead rows"
    dD = p.dD.clone()
    dD[~on] = 0
    h_nan = p.h.clone()
    h_nan[dead_rows] = float("nan")
    for acc in (0, 1):
        dh0 = p.dh0 if acc else None
        plain = _bwd_data(p, dD, p.W11, acc, dh0).live()
        out = _bwd_data(p, dD, p.W11, acc, dh0, live, row_last, row_step, rowB)
        flagged = out.live()
        assert torch.isfinite(flagged).all() and P.same_bits(flagged, plain), f"{name} accumulate {acc}: flags changed dh"
        rows = flagged.reshape(c.B, -1)[dead_rows]
        assert P.same_bits(rows, p.dh0.reshape(c.B, -1)[dead_rows]) if acc else not rows.any(), f"{name} accumulate {acc}: dh of dead rows"
        ref, S = R.drt_bwd_data(dD, p.W11, p.hmap, geo, c.nsel, dh0=dh0, on=on)
        _check("head_drt_bwd_data", f"{name}-flags-accumulate{acc}", out, ref, S, R.chain_drt_bwd_data(c.nsel, acc), GRAD, False)
    pW, pcs, _ = _bwd_weight(p, dD, p.h)
    fW, fcs, ws = _bwd_weight(p, dD, h_nan, live, row_last, row_step, rowB)
    assert torch.isfinite(fW.live()).all(), f"{name}: h of a dead row was read"
    assert P.same_bits(fW.live(), pW.live()) and P.same_bits(fcs.live(), pcs.live()), f"{name}: flags changed dW11 / dcbsum"
    slabs = ws.live().view(torch.int32).reshape(c.B, c.nsel, -1)
    for b in range(c.B):
        for i in range(c.nsel):
            assert bool((slabs[b, i] != P.SENTINEL).all()) == bool(on[i, b]), f"{name}: slab of row {b} slot {i}"


def test_sal_gather_bwd_does_not_read_dead_samples():
    c = R.Case("gather-dead-13x15", 13, 15, 5, 4, 3, 2, 64, "mixed")
    p = _problem(c, "gauss")
    dZ2, ldt, row_last = p.dZ2(), 114, [9, 2, 3, 9, 0]          # row_step = 3: sample 2 is alive
    dead = [1, 4]
    plain = _gather_bwd(p, dZ2, 2, ldt).live().reshape(c.B, -1)
    dZn = dZ2.clone()
    dZn[dead] = float("nan")
    flagged = _gather_bwd(p, dZn, 2, ldt, row_last, 3).live().reshape(c.B, -1)
    assert torch.isfinite(flagged).all() and not flagged[dead].any()
    assert P.same_bits(flagged[[0, 2, 3]], plain[[0, 2, 3]])


def test_num_classes_on_every_side():
    _, L = P.abi()
    for side in range(1, 171):
        for Hm, Wm in ((side, 13), (13, side), (side, side)):
            assert L.sp_head_num_classes(Hm, Wm) == R.num_classes(Hm, Wm), (Hm, Wm)
            want = -1 if R.num_classes(Hm, Wm) < 0 else 2 * 3 * R.num_classes(Hm, Wm) * 121 * 8 * 4
            assert L.sp_drt_direct_bwd_weight_workspace(2, Hm, Wm, 8, 3) == want, (Hm, Wm)
    for side in (1, 2, 163, 164, 170):
        assert L.sp_head_num_classes(side, 40) == -1 and L.sp_head_num_classes(40, side) == -1


# ====================================================================================================================
# refusals: one row per `return SP_ENULL` / `SP_EINVAL` of the file
# ====================================================================================================================
_DEF = dict(nheads=1, HC=64, C=4, Hm=7, Wm=8, B=2, ldt=50, nsel=1, nsrc=1, accumulate=0, row_step=0, rowB=0)
_ENTRIES = {      # name -> (arguments in order, input pointers, output pointers, optional pointers)
    "sp_head_compose11_fwd": ("G cb nheads HC C Hm Wm W11 cbsum", "G cb", "W11 cbsum", ""),
    "sp_head_compose11_bwd": ("dW11 dcbsum nheads HC C Hm Wm dG dcb", "dW11 dcbsum", "dG dcb", ""),
    "sp_sal_gather_fwd": ("T B Hm Wm ldt nsel hmap Z2", "T hmap", "Z2", ""),
    "sp_sal_gather_bwd": ("dZ2 B Hm Wm ldt nsel nsrc hmap dT row_last row_step", "dZ2 hmap", "dT", "row_last"),
    "sp_drt_direct_fwd": ("h W11 cbsum hmap B Hm Wm C nsel Dpre", "h W11 cbsum hmap", "Dpre", ""),
    "sp_drt_direct_bwd_data": ("dDpre W11 hmap B Hm Wm C nsel accumulate dh live row_last row_step rowB", "dDpre W11 hmap", "dh", "live row_last"),
    "sp_drt_direct_bwd_weight": ("dDpre h hmap B Hm Wm C nsel nheads workspace dW11 dcbsum live row_last row_step rowB", "dDpre h hmap",
                                 "workspace dW11 dcbsum", "live row_last"),
}
_SHAPE = [("C-not-4", dict(C=6)), ("B0", dict(B=0)), ("nsel0", dict(nsel=0)), ("nheads0", dict(nheads=0)), ("nsrc0", dict(nsrc=0)), ("HC50", dict(HC=50)),
          ("Hm2", dict(Hm=2)), ("Wm2", dict(Wm=2)), ("Hm163", dict(Hm=163)), ("Wm163", dict(Wm=163)), ("ldt49", dict(ldt=49)),
          ("ldt-below-50-nsrc", dict(nsrc=2, ldt=99)), ("row_last-rowB0", dict(row_last=True, rowB=0)), ("row_last-B-not-rowB", dict(B=4, row_last=True, rowB=3))]
# which shape rows each entry point refuses (the gathers take any map; only the drt entries know rowB)
_APPLIES = {
    "sp_head_compose11_fwd": "C-not-4 nheads0 HC50 Hm2 Wm2 Hm163 Wm163", "sp_head_compose11_bwd": "C-not-4 nheads0 HC50 Hm2 Wm2 Hm163 Wm163",
    "sp_sal_gather_fwd": "B0 nsel0 ldt49", "sp_sal_gather_bwd": "B0 nsel0 nsrc0 ldt49 ldt-below-50-nsrc",
    "sp_drt_direct_fwd": "C-not-4 B0 nsel0 Hm2 Wm2 Hm163 Wm163",
    "sp_drt_direct_bwd_data": "C-not-4 B0 nsel0 Hm2 Wm2 Hm163 Wm163 row_last-rowB0 row_last-B-not-rowB",
    "sp_drt_direct_bwd_weight": "C-not-4 B0 nsel0 nheads0 Hm2 Wm2 Hm163 Wm163 row_last-rowB0 row_last-B-not-rowB",
}
REFUSALS = []
for _fn, (_args, _ins, _outs, _opt) in _ENTRIES.items():
    REFUSALS += [(_fn, f"{_n}-null", {}, _n, ENULL) for _n in (_ins + " " + _outs).split()]
    REFUSALS += [(_fn, _row, _over, None, EINVAL) for _row, _over in _SHAPE if _row in _APPLIES[_fn].split()]


@pytest.mark.parametrize("fn,row,over,null,rc", REFUSALS, ids=[f"{r[0]}-{r[1]}" for r in REFUSALS])
def test_head_refusals(fn, row, over, null, rc):
    hip, L = P.abi()
    args, ins, outs, opt = (s.split() for s in _ENTRIES[fn])
    v = {**_DEF, **over}
    n = 1 << 15                                  # larger than every buffer of the default shape (and of the 4-row one)
    zeros, izeros = torch.zeros(n, device=P.dev()), torch.zeros(n, dtype=torch.int32, device=P.dev())
    bufs = {o: P.output(n) for o in outs}
    call = []
    for a in args:
        if a == null:
            call.append(None)
        elif a in outs:
            call.append(bufs[a].ptr)
        elif a in ins:
            call.append((izeros if a == "hmap" else zeros).data_ptr())
        elif a in opt:
            call.append(izeros.data_ptr() if v.get(a) else None)
        else:
            call.append(v[a])
    got = getattr(L, fn)(*call, hip.stream())
    torch.cuda.synchronize()
    assert got == rc, (fn, row, got)
    for o, b in bufs.items():
        assert b.untouched(), f"{fn} {row}: the refused call wrote {o}"

