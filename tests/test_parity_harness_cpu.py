"""The teeth of tests/parity.py, without a GPU: buffers on torch.device("cpu"), plain tensor writes standing in for a kernel.  Every check the parity
modules lean on -- guards, pads, finiteness, the element-wise bar, the lattice equality, the all-untouched check of a refused call -- must FAIL, with
its own message, on the one defect it is there for; two Summary objects share nothing; the fixture prints one line per group."""
import numpy as np
import pytest
import torch

import parity as P

CPU = torch.device("cpu")
CHAIN = 4
_summary = P.Summary("harness").fixture()          # as a module uses it (nothing is judged into this one: it prints its total line only)


def _case():
    """a batched, strided output (2 items of 3 x 5, ld 7, 4 words between the items) on the CPU with the reference written into it, and S.
    ref = 1 + k / 1024 and S = 1: bar = 2^-22 + 2^-149, and ref + 2^-21 is a float, so "twice the bar" below is exact"""
    out = P.Guarded(2, 3, 5, 7, 3 * 7 + 4, fill="sentinel")
    buf, ref = P.up(out, CPU), 1.0 + torch.arange(30, dtype=torch.float64).reshape(2, 3, 5) / 1024
    out.live(buf.dev).copy_(ref)
    return out, buf, ref, torch.ones_like(ref)


def test_judge_passes_the_reference_itself():
    out, buf, ref, S = _case()
    s = P.Summary("t")
    s.judge("g", "equal", out, buf.flat(), ref, S, CHAIN, legacy=1e-6)
    assert s.rows["g"] == [(0.0, "equal", 0.0, float(P.bar(1.0, CHAIN)), CHAIN)]
    assert buf.pads_untouched() and not buf.untouched() and torch.equal(buf.live().double(), ref)


OUTSIDE = "g case: a word outside the live output changed"
DEFECTS = [   # (id, index into the allocation or the live output, what is added there, the message judge fails with)
    ("guard-before", 0, 1.0, OUTSIDE), ("guard-after", -1, 1.0, OUTSIDE), ("row-pad", P.GUARD + 5, 1.0, OUTSIDE), ("batch-gap", P.GUARD + 22, 1.0, OUTSIDE),
    ("live-nan", (1, 2, 4), P.NAN, "a live output word is not finite"),
    ("twice-the-bar", (1, 0, 3), 2.0 ** -21, r"g case: err 4\.768e-07 > bar 2\.384e-07 at element 18 \(c = 4\)")]          # err / bar = 2 / (1 + 2^-127)


@pytest.mark.parametrize("where,add,message", [d[1:] for d in DEFECTS], ids=[d[0] for d in DEFECTS])
def test_judge_fails_on_one_defective_word(where, add, message):
    out, buf, ref, S = _case()
    if isinstance(where, tuple):
        out.live(buf.dev)[where] += add
    else:
        assert out.pad_mask()[where]
        buf.dev[where] = add
    with pytest.raises(AssertionError, match=message):
        P.Summary("t").judge("g", "case", out, buf.flat(), ref, S, CHAIN)
    if message == OUTSIDE:
        with pytest.raises(AssertionError, match="outside the live region"):
            buf.live()


def test_judge_holds_the_max_norm_bar_too_and_passes_half_a_bar():
    out, buf, ref, S = _case()
    out.live(buf.dev)[1, 0, 3] += 2.0 ** -23
    s = P.Summary("t")
    s.judge("g", "half", out, buf.flat(), ref, S, CHAIN, legacy=1e-6)
    assert s.rows["g"][0][0] == 0.5
    with pytest.raises(AssertionError, match="g case: max err"):          # 2^-19 is inside the element-wise bar at S = 8 and outside 1e-6 max|ref|
        s.judge("g", "case", out, buf.flat(), ref + 2.0 ** -19, 8 * S, CHAIN, legacy=1e-6)


def test_exact_fails_on_one_ulp_and_takes_either_zero():
    s, ref = P.Summary("t"), torch.tensor([[0.0, 1.0, -3.0]], dtype=torch.float64)
    s.exact("g", "zeros", torch.tensor([[-0.0, 1.0, -3.0]]), ref)
    with pytest.raises(AssertionError, match=r"g ulp: 1 words differ from the exact result, first at \[0, 1\]: 1\.00000011920\d* != 1\.0"):
        s.exact("g", "ulp", torch.tensor([[0.0, 1.0 + 2.0 ** -23, -3.0]]), ref)


def test_a_refused_call_that_wrote_one_word_is_seen():
    buf = P.output(40, device=CPU)
    assert buf.untouched() and (buf.read() == P.SENTINEL).all()
    buf.dev[P.GUARD + 7] = 0.0
    assert not buf.untouched() and buf.pads_untouched()          # a live word: only the all-untouched check sees it
    r = P.raw(8, init=np.array([1.5, -2.0], np.float32), device=CPU)
    assert r.untouched() and (r.read().view(np.float32) == [1.5, -2.0]).all() and r.ptr == r.dev.data_ptr() + 4 * P.GUARD
    r.dev[-1] = 0.0
    with pytest.raises(AssertionError, match="outside the live region"):
        r.read()
    op = P.operand(torch.arange(6.0), CPU)
    assert P.operand(None) is None and P.at(None) is None and P.at(op, 8) == op.ptr + 8
    assert torch.isnan(op.dev[:P.GUARD]).all() and torch.isnan(op.dev[-P.GUARD:]).all() and torch.equal(op.live().reshape(-1), torch.arange(6.0))


def _judge_rows(s, group, errs):
    """one comparison per entry of errs under the names r0, r1, ...: a float next to 1 moves in steps of 2^-23, half the bar"""
    for k, e in enumerate(errs):
        ref = torch.ones(1, 1, 4, dtype=torch.float64)
        got = ref.float()
        got[0, 0, 2] += e * 2.0 ** -23
        s.judge_values(group, f"r{k}", got, ref, torch.ones_like(ref), CHAIN)


def test_two_summaries_share_no_rows():
    a, b = P.Summary("a"), P.Summary("b")
    _judge_rows(a, "g", [1, 0])
    _judge_rows(b, "h", [1])
    assert {k: len(v) for k, v in a.rows.items()} == {"g": 2} and {k: len(v) for k, v in b.rows.items()} == {"h": 1}


def test_fixture_prints_one_line_per_group_in_the_given_order_with_the_worst_row(capsys):
    s = P.Summary("harness", ("second", "first", "never-judged"))
    fix = s.fixture()
    run = (getattr(fix, "__wrapped__", None) or fix.__pytest_wrapped__.obj)()          # the generator under pytest's fixture object
    next(run)
    _judge_rows(s, "first", [0, 2, 1])
    _judge_rows(s, "second", [1, 0])
    _judge_rows(s, "late", [0])                      # a group the order does not name comes after the named ones
    with pytest.raises(StopIteration):
        next(run)
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("PARITY-SUMMARY")]
    assert lines[:2] == ["PARITY-SUMMARY second: 2 comparisons, worst err/bar 0.500 at r0 (err 1.19e-07, bar 2.38e-07, c 4)",
                         "PARITY-SUMMARY first: 3 comparisons, worst err/bar 1.000 at r1 (err 2.38e-07, bar 2.38e-07, c 4)"]
    assert lines[2].startswith("PARITY-SUMMARY late: 1 comparisons, worst err/bar 0.000 at r0 ")
    assert len(lines) == 4 and lines[3].startswith("PARITY-SUMMARY harness total ") and lines[3].endswith(" s")
    P.Summary().report(0.04)
    assert capsys.readouterr().out == "\nPARITY-SUMMARY total 0.0 s\n"
