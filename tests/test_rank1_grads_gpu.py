"""sp_rank1_grads_f16x2 (csrc/rank1_grads.hip) through the C ABI against tests/rank1_grads_ref.py (held to torch.bmm in fp64 and to its own
claims by tests/test_rank1_grads_ref_cpu.py): one tile in total, exactly one chunk, a chunk and a tile more, one / two / three channel chunks, dense
and padded plane rows (fp16 NaN in the pad columns), dead samples, and taps that are Gaussian, on the lattice, spread over 2^-20 .. 1 inside a
chunk, all zero in a chunk, at 2^-120 (the tap scale clamps) and at 2^100.

dsp, dwc and the workspace (exactly sp_rank1_grads_workspace bytes) lie between sentinel guards; the taps between NaN guards.  Every live word is
finite and inside the ELEMENT-WISE bar against R_planes, and inside representation bound + bar against R_true; Gaussian operands also meet the 4e-6
max-norm bar of tests/test_ops_gpu.py; lattice data equals R_planes exactly (torch.equal in fp64).  Two launches are bit-identical.  Dead samples
(row_last): their planes are NaN, their dsp / dwc exact zeros, live samples bit-identical to the dense launch.  Every refusal leaves outputs and
workspace untouched and agrees with sp_rank1_grads_applies.  Each comparison prints a PARITY line, the module a summary per group
(profiles/rank1_grads_parity.md)."""
import functools

import numpy as np
import pytest
import torch

import parity as P
import rank1_grads_ref as R

pytestmark = pytest.mark.gpu

SUM = P.Summary("rank1", ("rank1_dsp", "rank1_dwc"))
_summary = SUM.fixture()
_problem = functools.lru_cache(maxsize=None)(R.Problem)          # case -> operands and restatement, built once


def _launch(p, planes, flags):
    """one launch on fresh buffers -> (dsp [B, P, KP], dwc [B, N3, KP]) on the host, guards and workspace bounds checked"""
    hip, L = P.abi()
    c = p.c
    Y, W, sy, sw = P.u16(planes), P.u16(p.Wp), P.f32([p.sy]), P.f32(p.sw)
    dT = P.operand(torch.from_numpy(p.taps))
    dsp, dwc = P.output(c.B * c.P * c.KP), P.output(c.B * c.N3 * c.KP)
    nbytes = L.sp_rank1_grads_workspace(c.B, c.P, c.N3, c.KP)
    assert nbytes == 4 * c.B * p.chunks * (c.N3 * c.KP + 1), nbytes
    ws = P.raw(nbytes)
    rl = torch.from_numpy(p.row_last).to(P.dev()) if flags else None
    assert L.sp_rank1_grads_applies(c.B, c.P, c.N3, c.KP, c.ldy) == 1
    rc = L.sp_rank1_grads_f16x2(Y.data_ptr(), sy.data_ptr(), c.ldy, W.data_ptr(), sw.data_ptr(), dT.ptr, c.B, c.P, c.N3, c.KP, dsp.ptr, dwc.ptr,
                                ws.ptr, None if rl is None else rl.data_ptr(), p.row_step, hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, (c.name, rc)
    ws.live()
    return dsp.live().reshape(c.B, c.P, c.KP), dwc.live().reshape(c.B, c.N3, c.KP)


@pytest.mark.parametrize("case", R.cases(), ids=lambda c: c.name)
def test_rank1_grads(case):
    p, c = _problem(case), case
    dsp, dwc = _launch(p, p.Yp, False)
    for group, got, (ref, S), chain, true, rep in (("rank1_dsp", dsp, p.dsp_planes(), p.chain_dsp, p.dsp_true(), p.dsp_rep()),
                                                   ("rank1_dwc", dwc, p.dwc_planes(), p.chain_dwc, p.dwc_true(), p.dwc_rep())):
        SUM.judge_values(group, c.name, got, ref, S, chain)
        assert ((got.double() - true).abs() <= rep + P.bar(S, chain)).all(), f"{group} {c.name}: outside the representation bound of the true product"
        # the max-norm bar of test_rank1_grads_kernel_gives_both_gradients_of_the_rank1_gate_term, where the group's own operands are Gaussian
        # (the taps enter dwc alone: under every kind but lattice and rows dsp is a product of Gaussian dpre and wc)
        if c.kind == "gauss" or (group == "rank1_dsp" and c.kind not in ("lattice", "rows")):
            e = float((got.double() - true).abs().max()) / float(true.abs().max())
            print(f"PARITY {group} {c.name}: relative max-norm error {e:.2e}")
            assert e <= 4e-6, (group, c.name, e)
        if c.kind == "lattice":
            assert max(p.exact_spans()) <= 2.0 ** 24
            SUM.exact(group, c.name, got, ref)
        if c.kind == "zero-all" and group == "rank1_dwc":
            assert not got.any()
    d2, w2 = _launch(p, p.Yp, False)
    assert P.same_bits(dsp, d2) and P.same_bits(dwc, w2), f"{c.name}: two launches differ"
    if p.dead:
        d3, w3 = _launch(p, p.planes_with_dead_rows_nan(), True)
        live = [b for b in range(c.B) if b not in p.dead]
        assert torch.isfinite(d3).all() and torch.isfinite(w3).all(), f"{c.name}: a dead sample's rows were read"
        assert not d3[p.dead].any() and not w3[p.dead].any(), f"{c.name}: a dead sample's gradients are not zeros"
        assert P.same_bits(d3[live], dsp[live]) and P.same_bits(w3[live], dwc[live]), f"{c.name}: live samples differ from the dense launch"


@pytest.mark.parametrize("r", R.refusals(), ids=lambda r: r.name)
def test_rank1_refusals(r):
    hip, L = P.abi()
    assert L.sp_rank1_grads_applies(r.B, r.P, r.N3, r.KP, r.ldy) == r.applies, r.name
    n = 1 << 16                                     # every buffer is large enough for the shape a refusal row names (B = 65536 is refused first)
    Y, W, sy, sw, taps = P.u16(np.zeros(2 * n, np.uint16)), P.u16(np.zeros(2 * n, np.uint16)), P.f32([1.0]), P.f32(np.ones(64)), P.f32(np.zeros(n))
    dsp, dwc, ws = P.raw(4 * 4096), P.raw(4 * 8192), P.raw(4 * 16384)
    ptrs = {"dpre_planes": Y.data_ptr() + r.offY, "dpre_scale": sy.data_ptr(), "wcT_planes": W.data_ptr() + r.offW, "wcT_row_scale": sw.data_ptr(),
            "spcol": taps.data_ptr(), "dsp": dsp.ptr, "dwc": dwc.ptr, "workspace": ws.ptr + r.offWs}
    if r.null:
        ptrs[r.null] = None
    rc = L.sp_rank1_grads_f16x2(ptrs["dpre_planes"], ptrs["dpre_scale"], r.ldy, ptrs["wcT_planes"], ptrs["wcT_row_scale"], ptrs["spcol"], r.B, r.P, r.N3,
                                r.KP, ptrs["dsp"], ptrs["dwc"], ptrs["workspace"], None, 0, hip.stream())
    torch.cuda.synchronize()
    assert rc == r.rc, (r.name, rc)
    assert dsp.untouched() and dwc.untouched() and ws.untouched(), f"{r.name}: a refused call wrote"
