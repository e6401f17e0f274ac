"""What the ops of functional.py tell each other through the tensors that pass between them: one declared record per tensor
(attribute ``_sp``), written by a producer, read by a consumer several autograd nodes away.  The slots below are the whole list.

Two rules:
  * A GRADIENT HINT rides on a tensor that a backward returns.  Autograd does not guarantee that object's identity (a hook, an
    accumulation, a cloning wrapper), so a hint may be lost, and losing it must only make a pass dense or slow, never wrong.
  * Anything whose loss WOULD be wrong goes through a token captured in forward instead: _FanOut's token, filled by alias index, and
    _Conv2d's dy_token.  A FORWARD-VALUE note stays on the object it was set on (an output created inside Function.forward keeps
    it through apply; functional._h_dest covers the one case that does not).
"""


class Notes:
    __slots__ = (      # kind: meaning | written by -> read by
        "amax",        # value, hint: {scale, max|t| bits} | _BnAct(Split), _FanOut fan-ins, cells (h, dpre, dcp) -> split_op, bn_act, cell bwd
        "cache",       # value, hint: {scheme: SplitOperand}, ONE dict for all aliases, {} = split once | _BnActSplit, cells -> split_op, convs
        "cbound",      # value: bound of max|c_t| on the cell state | _cell_bounds -> _cell_bounds of the next step
        "bnstats",     # value: first BatchNorm statistics stage, done by the conv epilogue | _Conv2d.forward -> bn_act
        "from_split",  # value: the conv ran from the 2xfp16 operand, its backward reads a split gradient | _Conv2d.forward -> bn_act
        "dy_token",    # value: the conv's backward reads ONLY the split gradient (the token is the guard) | _Conv2d.forward -> bn_act
        "uninit",      # value: fp32 form allocated, never written (skip_z) | _BnActSplit.forward -> _Conv2d.forward (refusal)
        "fan",         # value: (token, i) of fan-out alias i | fanout -> cell forwards (ctx.fan)
        "fan_ev",      # value: (events, i) of fan-out alias i | fanout -> _GateConvLstm.forward (ctx.h_events)
        "skipped",     # hint: fp32 form of this gradient never written | _lstm_rank1_backward -> _fp32_required, _FanOut.backward
        "rows",        # hint: (rows_ctx, step), dead samples' rows are exact zeros | _SemPool.backward -> _FanOut.backward
        "live",        # hint: flags [nsel][B] of non-zero duration gradients | _DrtHeadsBatched.backward -> _DrtDirect.backward
    )

    def __init__(self):
        self.amax = self.cache = self.cbound = self.bnstats = self.dy_token = self.fan = self.fan_ev = self.rows = self.live = None
        self.from_split = self.uninit = self.skipped = False


class _Default(Notes):
    __slots__ = ()

    def __setattr__(self, name, value):
        raise AttributeError("scanpaths_amd: the shared default Notes is read-only; writers use note(t), not notes(t)")


_DEFAULT = Notes()
_DEFAULT.__class__ = _Default          # filled, then frozen


def notes(t) -> Notes:
    """t's record for READING: the shared all-default one when t is None or carries none (nothing is allocated or attached)"""
    return getattr(t, "_sp", _DEFAULT)


def note(t) -> Notes:
    """t's record for WRITING, attached on first use: note(y).amax = hint"""
    n = getattr(t, "_sp", None)
    if n is None:
        n = t._sp = Notes()
    return n


def carry(src, outs, fields=("cache", "amax")):
    """aliases of src (fanout, tap) inherit these fields: each alias gets its own record, the cache dict is shared by reference"""
    for f in fields:
        v = getattr(notes(src), f)
        if v is not None:
            for o in outs:
                setattr(note(o), f, v)
