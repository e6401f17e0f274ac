"""CPU-only checks of scanpaths_amd/notes.py, the declared record through which the ops of functional.py tell each other things on the
tensors that pass between them, and of the host code that moves it (fanout, tap, _fp32_required, _cell_bounds).  No device: the
forwards of _FanOut / _Tap are view_as only."""
import os
import re

import pytest
import torch

from scanpaths_amd.notes import Notes, note, notes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("amax", "cache", "cbound", "bnstats", "from_split", "dy_token", "uninit", "fan", "fan_ev", "skipped", "rows", "live")


def test_notes_declares_exactly_its_fields_and_refuses_others():
    n = Notes()
    assert Notes.__slots__ == FIELDS and not hasattr(n, "__dict__")
    for f in FIELDS:
        assert getattr(n, f) is (False if f in ("from_split", "uninit", "skipped") else None), f
    with pytest.raises(AttributeError):
        n.amx = 1                      # a misspelt name must not silently turn a fusion (or a safety check) off
    with pytest.raises(AttributeError):
        n.split_grad_ok = True         # the dead mark is gone


def test_reading_allocates_nothing_and_the_default_record_is_frozen():
    t = torch.zeros(4)
    d = notes(t)
    assert d is notes(t) is notes(None) and isinstance(d, Notes)
    assert not hasattr(t, "_sp")
    for f in FIELDS:
        assert getattr(d, f) is getattr(Notes(), f), f
        with pytest.raises(AttributeError):
            setattr(d, f, 1)           # a writer that used notes() instead of note() is caught
    n = note(t)
    assert n is not d and n is note(t) is notes(t) and t._sp is n
    n.amax = 3
    assert notes(t).amax == 3 and notes(None).amax is None


@pytest.mark.parametrize("numel", [32, 24])
def test_fanout_and_tap_carry_cache_and_amax_to_every_alias(numel):
    from scanpaths_amd import functional as F
    x = torch.arange(float(numel)).view(2, numel // 2).requires_grad_(True)
    hint, cache = torch.ones(2), {"f16x2": object()}
    note(x).amax, note(x).cache = hint, cache
    outs = F.fanout(x, 3, step=None)
    taps = F.tap(x, F.GradMerge())
    assert len(outs) == 3 and len(taps) == 2
    for o in outs + taps:
        assert notes(o).amax is hint and notes(o).cache is cache and torch.equal(o, x)
    recs = [notes(o) for o in outs + taps] + [notes(x)]
    assert len({id(r) for r in recs}) == len(recs)          # fan / fan_ev differ per alias: one record each
    if numel % 16 == 0:
        token = notes(outs[0]).fan[0]
        assert token == {} and all(notes(o).fan[0] is token and notes(o).fan == (token, i) for i, o in enumerate(outs))
    else:
        assert all(notes(o).fan is None for o in outs)
    assert all(notes(o).fan_ev is None for o in outs) and all(notes(o).fan is None for o in taps)
    # a tensor without notes: nothing to carry, and reading makes no record
    y = torch.zeros(3, 5, requires_grad=True)
    assert all(not hasattr(o, "_sp") for o in F.fanout(y, 2) + F.tap(y, F.GradMerge()))


def test_fp32_required_refuses_a_skipped_gradient_and_passes_its_clone():
    from scanpaths_amd import functional as F
    g = torch.zeros(8)
    F._fp32_required(g, "test")
    note(g).skipped = True
    with pytest.raises(RuntimeError, match="exists only as a split operand"):
        F._fp32_required(g, "test")
    F._fp32_required(g.clone(), "test")          # a gradient hint does not survive a new tensor object


def test_cell_bounds_travel_on_the_state_tensor():
    from scanpaths_amd import functional as F
    c, c2, c3 = torch.zeros(2), torch.zeros(2), torch.zeros(2)
    assert F._cell_bounds(None, c) == (1.0, 0.0) and notes(c).cbound == 1.0
    assert F._cell_bounds(c, c2) == (2.0, 1.0) and notes(c2).cbound == 2.0
    assert F._cell_bounds(torch.zeros(2), c3) == (None, None) and not hasattr(c3, "_sp")


def test_no_ad_hoc_tensor_attribute_is_left_in_the_package():
    """every note goes through notes.py; `_sp_flat` is FlatAdam's mark on a parameter, not a note"""
    hits = []
    for d, _, files in os.walk(os.path.join(ROOT, "scanpaths_amd")):
        for f in files:
            if f.endswith((".so", ".o", ".pyc")):
                continue
            for i, line in enumerate(open(os.path.join(d, f), errors="replace"), 1):
                hits += [f"{f}:{i}: {m}" for m in re.findall(r"_sp_[a-z]\w*", line) if m != "_sp_flat"]
    assert not hits, hits
