"""The pooling, layout, column-sum and fan-in entry points of csrc/bn_pool.hip -- sp_maxpool3s2_fwd / bwd, sp_colsum with its workspace query, sp_sum_n
(dense and row-sparse), sp_sum_n_mixed, sp_nchw_to_nhwc_pad, sp_pad_lastdim, sp_add, sp_relu_bwd -- through the C ABI against tests/pool_sum_ref.py
(held to torch's fp64 max_pool2d and to its own claims by tests/test_pool_sum_ref_cpu.py), at the sizes where their launch rules change: one and two
grid-stride passes, the one-launch / two-stage switch of sp_colsum and every edge of its second stage's unrolled rounds, 1 .. 32 terms, whole and
partial float4 / 16-element groups, padded rows.

Every operand lies between NaN guards, every output, workspace (exactly the queried size) and amax word between sentinel guards, and every
comparison goes through Buffer.live(): a guard, pad or gap word that changed fails the test.  Pooling values and bytes, both layout copies, sp_add
and sp_relu_bwd are EXACT (bit for bit).  The sums meet the rounded-once bar -- measured against |ref|, on data that cancels seven orders, where an
fp32 accumulation fails by >= 100x -- sp_colsum with beta = 1 the rounded-twice bar, the pooling backward c = 4; lattice data equal the fp64 result
word for word.  The two-stage column sum and the three fan-ins run twice: identical bits.  Dead (term, sample) pairs hold NaN and are not read; a
refused call leaves every output untouched.  Each comparison prints a PARITY line, the module a summary per group (profiles/pool_sum_parity.md)."""
import ctypes as C

import numpy as np
import pytest
import torch

import parity as P
import pool_sum_ref as R

pytestmark = pytest.mark.gpu

SUM = P.Summary("pool_sum", ("maxpool_bwd", "colsum_beta0", "colsum_beta1", "sum_n", "sum_n_rows", "sum_n_mixed", "sum_n_mixed_rows"))
_summary = SUM.fixture()
F32, F64, I32 = np.float32, np.float64, np.int32
EINVAL, ENULL = -1, -2


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).reshape(-1).view(I32)


def words(a):
    """any array whose bytes are whole words -> an fp32 tensor of the same bytes (an operand that is not fp32: position bytes, fp16 planes, ints)"""
    return T(np.ascontiguousarray(a).reshape(-1).view(F32))


def done(rc, what, want=0):
    torch.cuda.synchronize()
    assert rc == want, (what, rc)


def ptrs(bufs, extra=0):
    return (C.c_void_p * len(bufs))(*[None if b is None else b.ptr + extra for b in bufs])


def amax_bits(out):
    return int(np.abs(out).max().astype(F32).reshape(1).view(I32)[0]) if out.size else 0


# ---- pooling ---------------------------------------------------------------------------------------------------------------------------------------
def _pool_fwd(L, hip, c, x, with_bytes):
    Ho, Wo = R.out_size(c.H), R.out_size(c.W)
    n = c.N * Ho * Wo * c.C
    X, Y, A = P.operand(T(x)), P.output(n), P.raw(n) if with_bytes else None
    done(L.sp_maxpool3s2_fwd(X.ptr, c.N, c.H, c.W, c.C, Y.ptr, P.at(A), Ho, Wo, hip.stream()), c.name)
    return Y.read(), None if A is None else A.read().view(np.uint8)


def _pool_bwd(L, hip, c, dy, pos):
    Ho, Wo = R.out_size(c.H), R.out_size(c.W)
    D, A, DX = P.operand(T(dy)), P.operand(words(pos)), P.output(c.N * c.H * c.W * c.C)
    done(L.sp_maxpool3s2_bwd(D.ptr, A.ptr, c.N, c.H, c.W, c.C, DX.ptr, Ho, Wo, hip.stream()), c.name)
    return DX.live().reshape(c.N, c.H, c.W, c.C)


@pytest.mark.parametrize("c", R.pool_cases(), ids=lambda c: c.name)
def test_maxpool(c):
    hip, L = P.abi()
    x, dy = R.pool_data(c)
    y, pos = R.pool_fwd(x)
    got_y, got_pos = _pool_fwd(L, hip, c, x, True)
    assert np.array_equal(got_y, bits(y)), f"{c.name}: y differs from the restatement in {(got_y != bits(y)).sum()} words"
    assert np.array_equal(got_pos, pos.reshape(-1)), f"{c.name}: {(got_pos != pos.reshape(-1)).sum()} window positions differ"
    y_alone, _ = _pool_fwd(L, hip, c, x, False)
    assert np.array_equal(y_alone, got_y), f"{c.name}: argmax = NULL changes y"
    ref, S = T(R.pool_bwd(dy, pos, c.H, c.W)), T(R.pool_bwd(np.abs(dy), pos, c.H, c.W))
    for whose, p in (("own-bytes", got_pos), ("ref-bytes", pos.reshape(-1))):          # the chain, and the backward alone
        dx = _pool_bwd(L, hip, c, dy, p)
        SUM.judge_values("maxpool_bwd", f"{c.name}-{whose}", dx, ref, S, 4)
        if c.kind == "int":
            SUM.exact("maxpool_bwd", f"{c.name}-{whose}", dx, ref)
    if c.kind == "nan":
        assert np.isnan(y[0, 0, 0, 0]) and got_pos.reshape(pos.shape)[0, 1, 1, 0] == 5


def test_maxpool_refusals():
    hip, L = P.abi()
    X, Y, A, D, DX = P.operand(torch.zeros(4096)), P.output(4096), P.raw(4096), P.operand(torch.zeros(4096)), P.output(4096)
    s = hip.stream()
    done(L.sp_maxpool3s2_fwd(X.ptr, 1, 5, 5, 6, Y.ptr, A.ptr, 2, 2, s), "fwd C % 4", EINVAL)
    done(L.sp_maxpool3s2_fwd(None, 1, 5, 5, 8, Y.ptr, A.ptr, 2, 2, s), "fwd x NULL", ENULL)
    done(L.sp_maxpool3s2_fwd(X.ptr, 1, 5, 5, 8, None, A.ptr, 2, 2, s), "fwd y NULL", ENULL)
    done(L.sp_maxpool3s2_bwd(D.ptr, X.ptr, 1, 5, 5, 6, DX.ptr, 2, 2, s), "bwd C % 4", EINVAL)
    done(L.sp_maxpool3s2_bwd(None, X.ptr, 1, 5, 5, 8, DX.ptr, 2, 2, s), "bwd dy NULL", ENULL)
    done(L.sp_maxpool3s2_bwd(D.ptr, None, 1, 5, 5, 8, DX.ptr, 2, 2, s), "bwd argmax NULL", ENULL)
    done(L.sp_maxpool3s2_bwd(D.ptr, X.ptr, 1, 5, 5, 8, None, 2, 2, s), "bwd dx NULL", ENULL)
    assert Y.untouched() and A.untouched() and DX.untouched()


# ---- column sums -----------------------------------------------------------------------------------------------------------------------------------
def _colsum(L, hip, c, X, ld, old, beta):
    """one sp_colsum launch: x as uploaded (X; the launch only reads it), out and the workspace -- exactly the queried bytes -- fresh"""
    nbytes = L.sp_colsum_workspace(c.M, c.C)
    assert nbytes == R.pick_G(c.M, c.C) * c.C * 8, (c.name, nbytes)
    O, W = P.output(c.C, T(old) if beta else None), P.raw(nbytes)
    done(L.sp_colsum(X.ptr, c.M, c.C, ld, O.ptr, beta, W.ptr, hip.stream()), c.name)
    W.live()
    return O.live().reshape(-1)


@pytest.mark.parametrize("c", R.colsum_cases(), ids=lambda c: c.name)
def test_colsum(c):
    hip, L = P.abi()
    x, old = R.colsum_data(c)
    for dld, beta, off in R.COLSUM_VARIANTS:
        name, ld = f"{c.name}-ld+{dld}-beta{beta}-off{off}", c.C + dld
        X = P.up(P.Guarded(1, c.M, c.C, ld, fill="nan", data=T(x), offset=off))                # NaN in the pad columns of every row
        got = _colsum(L, hip, c, X, ld, old, beta)
        ref, Sp, _, _ = R.colsum_ref(x, old, beta)
        SUM.judge_values(f"colsum_beta{beta}", name, got, T(ref), T(Sp), 1)
        if c.kind in ("lattice", "wide"):
            SUM.exact(f"colsum_beta{beta}", name, got, T(ref))
        if R.colsum_path(c.M) == "two-stage":
            assert P.same_bits(got, _colsum(L, hip, c, X, ld, old, beta)), f"{name}: two launches differ"
        assert X.untouched()


def test_colsum_refusals():
    hip, L = P.abi()
    X, O, W = P.operand(torch.zeros(4096)), P.output(64), P.raw(1 << 16)
    s = hip.stream()
    for what, (x, M, Cc, ld, out, ws), want in (("C % 4", (X.ptr, 8, 6, 8, O.ptr, W.ptr), EINVAL), ("ld % 4", (X.ptr, 8, 8, 10, O.ptr, W.ptr), EINVAL),
                                                ("M = 0", (X.ptr, 0, 8, 8, O.ptr, W.ptr), EINVAL), ("x NULL", (None, 8, 8, 8, O.ptr, W.ptr), ENULL),
                                                ("out NULL", (X.ptr, 8, 8, 8, None, W.ptr), ENULL), ("workspace NULL", (X.ptr, 8, 8, 8, O.ptr, None), ENULL),
                                                ("two-stage M = 0", (X.ptr, 0, 8, 8, O.ptr, W.ptr), EINVAL), ("two-stage C % 4", (X.ptr, 200, 6, 8, O.ptr, W.ptr), EINVAL)):
        for beta in (0, 1):
            done(L.sp_colsum(x, M, Cc, ld, out, beta, ws, s), what, want)
    assert O.untouched() and W.untouched()


# ---- fan-ins ---------------------------------------------------------------------------------------------------------------------------------------
def _sum_n(L, hip, terms, n, amax=True, row_last=None, steps=None, ns=0):
    """one sp_sum_n launch on fresh buffers -> (out fp32 numpy, the amax word or None)"""
    ops = [P.operand(T(t)) for t in terms]
    out, am = P.output(n), P.output(1, torch.zeros(1)) if amax else None
    rl = None if row_last is None else P.raw(4 * len(row_last), np.array(row_last, I32))
    st = None if steps is None else (C.c_int * len(steps))(*steps)
    done(L.sp_sum_n(ptrs(ops), len(terms), n, out.ptr, P.at(am), P.at(rl), st, ns, hip.stream()), "sp_sum_n")
    return out.live().reshape(-1).numpy(), None if am is None else int(am.read()[0])


def _judge_sum(group, name, got, ref, S, k, kind):
    SUM.judge_values(group, name, T(got), T(ref), T(R.rounded_once(ref, S, k)), 1)
    if kind in ("lattice", "wide"):
        SUM.exact(group, name, T(got), T(ref))


@pytest.mark.parametrize("c", R.sum_cases(), ids=lambda c: c.name)
def test_sum_n(c):
    hip, L = P.abi()
    terms = R.make_terms(c.kind, "sum-" + c.name, c.count, (c.n,))
    ref, S = R.f64_sum(terms)
    got, am = _sum_n(L, hip, terms, c.n)
    _judge_sum("sum_n", c.name, got, ref, S, c.count, c.kind)
    assert am == amax_bits(got), f"{c.name}: amax word {am:#x}, max |out| {amax_bits(got):#x}"
    again, am2 = _sum_n(L, hip, terms, c.n)
    assert np.array_equal(bits(got), bits(again)) and am2 == am, f"{c.name}: two launches differ"
    alone, _ = _sum_n(L, hip, terms, c.n, amax=False)
    assert np.array_equal(bits(got), bits(alone)), f"{c.name}: out_amax = NULL changes out"


def test_sum_n_amax_stays_zero_on_a_zero_output():
    hip, L = P.abi()
    for n in (4, 1028):
        t = (R.rng(f"zero-{n}").standard_normal(n) * 3).astype(F32)
        got, am = _sum_n(L, hip, [t, np.zeros(n, F32), -t], n)
        assert not bits(got).any() and am == 0


@pytest.mark.parametrize("c", R.rows_cases(), ids=lambda c: c.name)
def test_sum_n_rows(c):
    hip, L = P.abi()
    live = R.live_mask(c)
    terms = R.rows_data(c)
    zeroed = [np.where(live[i], t, F32(0)) for i, t in enumerate(terms)]
    poisoned = [np.where(live[i], t, F32(np.nan)) for i, t in enumerate(terms)]
    ref, S = R.f64_sum(zeroed)
    got, am = _sum_n(L, hip, poisoned, c.n, row_last=c.row_last, steps=c.steps, ns=c.nsamples)
    assert np.isfinite(got).all(), f"{c.name}: a dead term was read"
    _judge_sum("sum_n_rows", c.name, got, ref, S, c.count, c.kind)
    assert am == amax_bits(got)
    dense, _ = _sum_n(L, hip, zeroed, c.n)
    assert np.array_equal(bits(got), bits(dense)), f"{c.name}: differs from the dense launch on zero-filled copies"
    for b in range(c.nsamples):
        if not live[:, b * c.per].any():
            assert not bits(got[b * c.per:(b + 1) * c.per]).any(), f"{c.name}: sample {b} has no live term and is not all +0"
    again, _ = _sum_n(L, hip, poisoned, c.n, row_last=c.row_last, steps=c.steps, ns=c.nsamples)
    assert np.array_equal(bits(got), bits(again)), f"{c.name}: two launches differ"


def test_sum_n_refusals():
    hip, L = P.abi()
    s = hip.stream()
    ops = [P.operand(torch.zeros(64)) for _ in range(33)]
    out, am, rl = P.output(64), P.output(1, torch.zeros(1)), P.raw(16, np.zeros(4, I32))
    st = (C.c_int * 33)(*([0] * 33))
    call = lambda lst, k, n, r, t, ns: L.sp_sum_n(lst, k, n, out.ptr, am.ptr, r, t, ns, s)
    done(call(ptrs(ops), 0, 64, None, None, 0), "count 0", EINVAL)
    done(call(ptrs(ops), 33, 64, None, None, 0), "count 33", EINVAL)
    done(call(ptrs(ops), 2, 62, None, None, 0), "n % 4", EINVAL)
    done(call(ptrs([ops[0], None, ops[2]]), 3, 64, None, None, 0), "a NULL list entry", ENULL)
    done(call(None, 3, 64, None, None, 0), "inputs NULL", ENULL)
    done(L.sp_sum_n(ptrs(ops), 3, 64, None, am.ptr, None, None, 0, s), "out NULL", ENULL)
    done(call(ptrs(ops), 3, 64, rl.ptr, None, 4), "row_last without steps", ENULL)
    done(call(ptrs(ops), 3, 64, None, st, 4), "steps without row_last", ENULL)
    done(call(ptrs(ops), 3, 64, rl.ptr, st, 3), "n % nsamples", EINVAL)
    done(call(ptrs(ops), 3, 40, rl.ptr, st, 4), "(n / nsamples) % 4", EINVAL)
    done(call(ptrs(ops), 3, 64, rl.ptr, st, 0), "nsamples 0", EINVAL)
    assert out.untouched() and am.untouched()


def _sum_n_mixed(L, hip, m, n, f32, planes, amax=True, row_last=None, steps=None, ns=0, plane_off=0, per_check=None):
    """one sp_sum_n_mixed launch on fresh buffers; the fp32 tensor of a split term is absent (NULL)"""
    k = len(f32)
    fo = [None if t is None else P.operand(T(t)) for t in f32]
    po = [None if p is None else P.operand(words(p)) for p in planes]
    so = [None if s is None else P.operand(torch.tensor([s], dtype=torch.float32)) for s in m.scale]
    out, am = P.output(n), P.output(1, torch.zeros(1)) if amax else None
    rl = None if row_last is None else P.raw(4 * len(row_last), np.array(row_last, I32))
    st = None if steps is None else (C.c_int * len(steps))(*steps)
    done(L.sp_sum_n_mixed(ptrs(fo), ptrs(po, plane_off), ptrs(so), k, n, out.ptr, P.at(am), P.at(rl), st, ns, hip.stream()), "sp_sum_n_mixed")
    return out.live().reshape(-1).numpy(), None if am is None else int(am.read()[0])


@pytest.mark.parametrize("c", R.mixed_cases(), ids=lambda c: c.name)
def test_sum_n_mixed(c):
    hip, L = P.abi()
    m = R.Mixed(c)
    ref, S = m.ref()
    got, am = _sum_n_mixed(L, hip, m, c.n, m.f32, m.planes)
    _judge_sum("sum_n_mixed", c.name, got, ref, S, c.count, c.kind)
    assert am == amax_bits(got)
    again, am2 = _sum_n_mixed(L, hip, m, c.n, m.f32, m.planes)
    assert np.array_equal(bits(got), bits(again)) and am2 == am, f"{c.name}: two launches differ"
    alone, _ = _sum_n_mixed(L, hip, m, c.n, m.f32, m.planes, amax=False)
    assert np.array_equal(bits(got), bits(alone)), f"{c.name}: out_amax = NULL changes out"


@pytest.mark.parametrize("c", R.rows_cases(R.MIXED_ROWS_PER, R.MIXED_LISTS), ids=lambda c: c.name)
def test_sum_n_mixed_rows(c):
    hip, L = P.abi()
    m = R.Mixed(c)
    live = R.live_mask(c)
    nan16 = np.array([np.nan], np.float16).view(np.uint16)[0]
    grp = lambda i: live[i].reshape(-1, 1, 16)                                  # the mask in the planes' layout [group][plane][16]
    zf = [None if t is None else np.where(live[i], t, F32(0)) for i, t in enumerate(m.f32)]
    zp = [None if p is None else np.where(grp(i), p, np.uint16(0)) for i, p in enumerate(m.planes)]
    nf = [None if t is None else np.where(live[i], t, F32(np.nan)) for i, t in enumerate(m.f32)]
    npl = [None if p is None else np.where(grp(i), p, nan16) for i, p in enumerate(m.planes)]
    ref, S = m.ref(live)
    got, am = _sum_n_mixed(L, hip, m, c.n, nf, npl, row_last=c.row_last, steps=c.steps, ns=c.nsamples)
    assert np.isfinite(got).all(), f"{c.name}: a dead term was read"
    _judge_sum("sum_n_mixed_rows", c.name, got, ref, S, c.count, c.kind)
    assert am == amax_bits(got)
    dense, _ = _sum_n_mixed(L, hip, m, c.n, zf, zp)
    assert np.array_equal(bits(got), bits(dense)), f"{c.name}: differs from the dense launch on zero-filled copies"
    for b in range(c.nsamples):
        if not live[:, b * c.per].any():
            assert not bits(got[b * c.per:(b + 1) * c.per]).any(), f"{c.name}: sample {b} has no live term and is not all +0"
    again, _ = _sum_n_mixed(L, hip, m, c.n, nf, npl, row_last=c.row_last, steps=c.steps, ns=c.nsamples)
    assert np.array_equal(bits(got), bits(again)), f"{c.name}: two launches differ"


def test_sum_n_mixed_refusals():
    hip, L = P.abi()
    s = hip.stream()
    f = [P.operand(torch.zeros(64)) for _ in range(33)]
    pl = [P.operand(torch.zeros(64)) for _ in range(33)]
    sc = [P.operand(torch.ones(1)) for _ in range(33)]
    out, am, rl = P.output(64), P.output(1, torch.zeros(1)), P.raw(16, np.zeros(4, I32))
    st = (C.c_int * 33)(*([0] * 33))
    call = lambda fl, pls, scs, k, n, r, t, ns: L.sp_sum_n_mixed(fl, pls, scs, k, n, out.ptr, am.ptr, r, t, ns, s)
    none3 = ptrs([None] * 3)
    done(call(ptrs(f), ptrs(pl), ptrs(sc), 0, 64, None, None, 0), "count 0", EINVAL)
    done(call(ptrs(f), ptrs(pl), ptrs(sc), 33, 64, None, None, 0), "count 33", EINVAL)
    done(call(ptrs(f), ptrs(pl), ptrs(sc), 3, 56, None, None, 0), "n % 16", EINVAL)
    done(call(none3, ptrs(pl[:3], 8), ptrs(sc[:3]), 3, 64, None, None, 0), "a plane pointer off by 8 bytes", EINVAL)
    done(call(none3, ptrs([pl[0], None, pl[2]]), ptrs(sc[:3]), 3, 64, None, None, 0), "a term with neither form", ENULL)
    done(call(none3, ptrs(pl[:3]), ptrs([sc[0], None, sc[2]]), 3, 64, None, None, 0), "a split term without its scale", ENULL)
    done(call(None, ptrs(pl), ptrs(sc), 3, 64, None, None, 0), "inputs NULL", ENULL)
    done(call(ptrs(f), ptrs(pl), ptrs(sc), 3, 64, rl.ptr, None, 4), "row_last without steps", ENULL)
    done(call(ptrs(f), ptrs(pl), ptrs(sc), 3, 64, None, st, 4), "steps without row_last", ENULL)
    done(call(ptrs(f), ptrs(pl), ptrs(sc), 3, 64, rl.ptr, st, 3), "n % nsamples", EINVAL)
    done(call(ptrs(f), ptrs(pl), ptrs(sc), 3, 64, rl.ptr, st, 8), "per-sample size % 16", EINVAL)
    assert out.untouched() and am.untouched()


# ---- layout, add, ReLU gradient --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,Cc,H,W,Cp", R.NHWC_CASES, ids=lambda v: str(v))
def test_nchw_to_nhwc_pad(N, Cc, H, W, Cp):
    hip, L = P.abi()
    x = R.rng(f"nhwc-{N}-{Cc}-{H}-{W}-{Cp}").standard_normal((N, Cc, H, W)).astype(F32)
    x.reshape(-1)[::7] *= -0.0                                                 # some -0.0: a copy keeps the sign, the fill is +0.0
    X, Y = P.operand(T(x)), P.output(N * H * W * Cp)
    done(L.sp_nchw_to_nhwc_pad(X.ptr, N, Cc, H, W, Cp, Y.ptr, hip.stream()), "sp_nchw_to_nhwc_pad")
    assert np.array_equal(Y.read(), bits(R.nhwc_ref(x, Cp)))


def test_nchw_to_nhwc_pad_refuses_a_narrower_output():
    hip, L = P.abi()
    X, Y = P.operand(torch.zeros(256)), P.output(256)
    done(L.sp_nchw_to_nhwc_pad(X.ptr, 1, 4, 4, 4, 3, Y.ptr, hip.stream()), "Cp < C", EINVAL)
    done(L.sp_nchw_to_nhwc_pad(None, 1, 4, 4, 4, 4, Y.ptr, hip.stream()), "x NULL", ENULL)
    assert Y.untouched()


@pytest.mark.parametrize("rows,Cin,Cout", R.PAD_CASES, ids=lambda v: str(v))
def test_pad_lastdim(rows, Cin, Cout):
    hip, L = P.abi()
    x = R.rng(f"pad-{rows}-{Cin}-{Cout}").standard_normal((rows, Cin)).astype(F32)
    x.reshape(-1)[::5] *= -0.0
    X, Y = P.operand(T(x)), P.output(rows * Cout)
    done(L.sp_pad_lastdim(X.ptr, rows, Cin, Cout, Y.ptr, hip.stream()), "sp_pad_lastdim")
    if rows == 0:
        assert Y.untouched()
    assert np.array_equal(Y.read(), bits(R.pad_ref(x, Cout)))


@pytest.mark.parametrize("n", R.ADD_N)
def test_add(n):
    hip, L = P.abi()
    g = R.rng(f"add-{n}")
    a, b = (g.standard_normal(n) * 2.0 ** g.integers(-20, 20, n)).astype(F32), (g.standard_normal(n) * 2.0 ** g.integers(-20, 20, n)).astype(F32)
    b[::9] = -a[::9]                                                           # exact zeros, +0
    A, B, O = P.operand(T(a)), P.operand(T(b)), P.output(n)
    done(L.sp_add(A.ptr, B.ptr, O.ptr, n, hip.stream()), "sp_add")
    assert np.array_equal(O.read(), bits((T(a) + T(b)).numpy()))
    done(L.sp_add(A.ptr, None, O.ptr, n, hip.stream()), "b NULL", ENULL)


@pytest.mark.parametrize("n", R.RELU_N)
def test_relu_bwd(n):
    hip, L = P.abi()
    dy, y = R.relu_data(n)
    D, Y, DX = P.operand(T(dy)), P.operand(T(y)), P.output(n)
    done(L.sp_relu_bwd(D.ptr, Y.ptr, n, DX.ptr, hip.stream()), "sp_relu_bwd")
    assert np.array_equal(DX.read(), bits(R.relu_ref(dy, y)))
    fresh = P.output(n)
    done(L.sp_relu_bwd(D.ptr, None, n, fresh.ptr, hip.stream()), "y NULL", ENULL)
    assert fresh.untouched()
