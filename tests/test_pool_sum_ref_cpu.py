"""tests/pool_sum_ref.py held to its own claims, with no GPU: what tests/test_pool_sum_gpu.py compares the kernels of csrc/bn_pool.hip with must be
right, and its inputs must be able to tell a wrong kernel from a right one.

Pooling: the restatement equals torch's fp64 max_pool2d(3, 2, ceil_mode=True, return_indices=True) and its autograd on every case -- values,
indices mapped to window bytes, backward; NaN and -inf included -- the integer data tie, a last-maximum rule and a floor-mode size are told apart.
Sums: an fp32 accumulation misses the rounded-once bar by >= 100x on every cancelling case that CAN show it (three terms or more: the fp32 sum of
two numbers is their correctly rounded sum), one dead row read gives NaN, the lattice spans hold, the wide lattice catches an fp32 accumulation
under `exact`, the hand-built split planes decode to 2^-22 and add exactly in fp32, and pick_G gives the G every case was chosen for."""
import numpy as np
import pytest
import torch

import parity as P
import pool_sum_ref as R

F32, F64 = np.float32, np.float64
POOL = R.pool_cases()


def _torch_pool(x, dy):
    """torch fp64 on NCHW -> (y, bytes, dx) in NHWC"""
    t = torch.from_numpy(x.astype(F64)).permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y, idx = torch.nn.functional.max_pool2d(t, 3, 2, ceil_mode=True, return_indices=True)
    y.backward(torch.from_numpy(dy.astype(F64)).permute(0, 3, 1, 2).contiguous())
    W = x.shape[2]
    Ho, Wo = y.shape[2], y.shape[3]
    iy, ix = idx // W, idx % W
    pos = (iy - 2 * torch.arange(Ho).view(1, 1, Ho, 1)) * 3 + (ix - 2 * torch.arange(Wo).view(1, 1, 1, Wo))
    nhwc = lambda a: a.permute(0, 2, 3, 1).contiguous().numpy()
    return nhwc(y.detach()), nhwc(pos).astype(np.uint8), nhwc(t.grad)


@pytest.mark.parametrize("c", POOL, ids=lambda c: c.name)
def test_pool_restatement_is_torch_max_pool2d(c):
    x, dy = R.pool_data(c)
    y, pos = R.pool_fwd(x)
    ty, tpos, tdx = _torch_pool(x, dy)
    assert y.shape == ty.shape == (c.N, R.out_size(c.H), R.out_size(c.W), c.C)
    assert np.array_equal(y.astype(F64), ty, equal_nan=True)
    assert np.array_equal(pos, tpos)
    assert np.array_equal(R.pool_bwd(dy, pos, c.H, c.W), tdx)                 # at most four fp64 terms of fp32 numbers: exact in any order
    if c.kind == "nan":
        cnt = R.nan_count(x)
        assert cnt[0, 0, 0, 0] == 1 and np.isnan(y[0, 0, 0, 0]) and pos[0, 0, 0, 0] == 4 and x[0, 1, 2, 0] == 100.0     # NaN, then a larger finite value
        assert cnt[0, 1, 1, 0] == 2 and np.isnan(y[0, 1, 1, 0]) and pos[0, 1, 1, 0] == 5                               # the LAST NaN
        assert cnt[0, 1, 2, 2] == 1 and pos[0, 1, 2, 2] == 3
        assert y[0, 0, 1, 0] == 100.0 and np.isfinite(y[..., 1]).all() and np.isfinite(y[..., 3]).all()
        assert (np.isnan(y) == (cnt > 0)).all()
    if c.kind == "neginf":
        assert np.isneginf(y[0, 0, 0]).all() and not pos[0, 0, 0].any() and np.isneginf(y[..., 1]).all() and not pos[..., 1].any()
        dx = R.pool_bwd(dy, pos, c.H, c.W)
        assert np.array_equal(dx[:, 0::2, 0::2, 1][:, :y.shape[1], :y.shape[2]], dy[..., 1].astype(F64))      # dy lands on each window's first element


@pytest.mark.parametrize("c", [c for c in POOL if c.kind == "int"], ids=lambda c: c.name)
def test_integer_data_tie_and_a_last_maximum_rule_is_caught(c):
    x, _ = R.pool_data(c)
    y, pos = R.pool_fwd(x)
    windows, tied, first_is_not_last = R.tie_stats(x, pos)
    print(f"{c.name}: {windows} windows, {tied} tied ({100.0 * tied / windows:.0f} %), {first_is_not_last} with first != last maximum")
    assert tied >= 1
    if windows >= 96:
        assert 2 * tied >= windows and first_is_not_last >= 1
        ylast, plast = R.pool_fwd(x, "last")
        assert np.array_equal(y, ylast) and not np.array_equal(pos, plast)
        _, dy = R.pool_data(c)
        assert not np.array_equal(R.pool_bwd(np.ones_like(dy), pos, c.H, c.W), R.pool_bwd(np.ones_like(dy), plast, c.H, c.W))


def test_floor_mode_size_differs_on_every_even_side():
    for n in range(2, 1500):
        assert (R.out_size(n) != R.out_size_floor(n)) == (n % 2 == 0), n
    sides = {s for c in POOL for s in (c.H, c.W)}
    assert any(s % 2 == 0 for s in sides) and any(s % 2 for s in sides)
    H, W = R.POOL_BIG[1:3]
    assert R.out_size(H) * R.out_size(W) > R.EW_CAP * R.EW_BLOCK and H * W > 4 * R.EW_CAP * R.EW_BLOCK          # the second grid-stride pass


# ---- sums ------------------------------------------------------------------------------------------------------------------------------------------
def _ratio(got, ref, Sp):
    return float((np.abs(got.astype(F64) - ref) / P.bar(Sp, 1)).max())


def _check_terms(terms, kind, name):
    """the claims on one list of terms"""
    k = len(terms)
    ref, S = R.f64_sum(terms)
    Sp = R.rounded_once(ref, S, k)
    assert _ratio(ref.astype(F32), ref, Sp) <= 1.0, name                                       # the correctly rounded sum meets the bar
    if kind == "cancel" and k >= 3:
        q = _ratio(R.f32_in_order(terms), ref, Sp)
        assert q >= 100.0, (name, q)
    if kind == "gauss" and k >= 2:                                                             # the final rounding is not exact: the bar's first term bites
        assert _ratio(ref.astype(F32), ref, Sp) >= 0.5 and _ratio(np.nextafter(ref.astype(F32), F32(0)), ref, Sp) > 1.0, name
    if kind == "lattice":
        assert S.max() / 2.0 ** -11 <= 2.0 ** 24, name
        assert np.array_equal(R.f32_in_order(terms).astype(F64), ref)                          # ... and then fp32 sums are exact as well
    if kind == "wide":
        assert S.max() <= 2.0 ** 53 and np.abs(ref).max() <= 2.0 ** 24 and np.array_equal(ref, np.round(ref)), name
        assert np.array_equal(ref.astype(F32).astype(F64), ref)
        assert not np.array_equal(R.f32_in_order(terms).astype(F64), ref), name                # what Summary.exact would catch


@pytest.mark.parametrize("c", [c for c in R.sum_cases() if c.n < 10 ** 6], ids=lambda c: c.name)
def test_sum_n_data(c):
    terms = R.make_terms(c.kind, "sum-" + c.name, c.count, (c.n,))
    assert len(terms) == c.count and all(t.dtype == F32 and t.shape == (c.n,) for t in terms)
    _check_terms(terms, c.kind, c.name)


def test_sum_cases_reach_every_branch():
    big = R.EW_CAP * R.EW_BLOCK
    assert R.SUM_BIG[1] % 4 == 0 and R.SUM_BIG[1] // 4 > big and R.MIXED_BIG[1] % 16 == 0 and R.MIXED_BIG[1] // 16 > big
    assert {c.count for c in R.sum_cases()} == {1, 2, 3, 31, 32} and {c.n for c in R.sum_cases()} >= {4, 8, 1020, 1024, 1028}
    assert {c.n for c in R.mixed_cases()} >= {16, 32, 16 * 257} and {c.forms for c in R.mixed_cases()} == set(R.MIXED_LISTS)
    assert sorted(R.SPLIT_EXP) == list(range(-8, 13))
    assert R.ADD_N[-1] // 4 > big and R.ADD_N[-1] % 4 == 3 and R.RELU_N[-1] > big
    N, C, H, W, Cp = R.NHWC_CASES[-1]
    assert N * H * W * Cp > big and R.PAD_CASES[-1][0] * R.PAD_CASES[-1][2] > big


@pytest.mark.parametrize("c", [c for c in R.mixed_cases() if c.n < 10 ** 6], ids=lambda c: c.name)
def test_mixed_operands(c):
    m = R.Mixed(c)
    for i in range(c.count):
        assert (m.f32[i] is None) == R.is_split(c.forms, i) == (m.planes[i] is not None)
        if m.planes[i] is not None:
            s = m.scale[i]
            assert 2.0 ** -8 <= s <= 2.0 ** 12 and np.log2(s) == int(np.log2(s))
            assert m.planes[i].shape == (c.n // 16, 2, 16) and R.planes_sum_exact_in_f32(m.planes[i])
    ref, S = m.ref()
    Sp = R.rounded_once(ref, S, c.count)
    assert _ratio(ref.astype(F32), ref, Sp) <= 1.0
    vals = [v.astype(F32) for v in m.value]
    assert all(np.array_equal(v.astype(F64), w) for v, w in zip(vals, m.value))                # every term is an fp32 number
    if c.kind == "cancel" and c.count >= 3:
        assert _ratio(R.f32_in_order(vals), ref, Sp) >= 100.0
    if c.kind == "lattice":
        assert S.max() / 2.0 ** -11 <= 2.0 ** 24
    if c.kind == "wide":
        assert not np.array_equal(R.f32_in_order(vals).astype(F64), ref)


def test_split_planes_decode_to_2_to_the_minus_22_of_the_maximum():
    g = R.rng("split-decode")
    for e in R.SPLIT_EXP:
        s = 2.0 ** e
        x = (g.standard_normal(4096) * (5e3 / s)).astype(F32)
        x[:16] = 0.0
        p = R.split_planes(x, s)
        assert np.abs(R.decode_planes(p, s) - x.astype(F64)).max() <= 2.0 ** -22 * np.abs(x).max(), e
        assert R.planes_sum_exact_in_f32(p)
        lay = p.view(np.float16)
        assert np.array_equal(lay[3, 0].astype(F64), (x[48:64].astype(F64) * s).astype(np.float16).astype(F64))     # [group][plane][16]


ROWS = R.rows_cases() + R.rows_cases(R.MIXED_ROWS_PER, R.MIXED_LISTS)


@pytest.mark.parametrize("c", ROWS, ids=lambda c: c.name)
def test_rows_cases(c):
    live = R.live_mask(c)
    assert live.shape == (c.count, c.n)
    assert sorted(c.steps) != list(c.steps) and ((-1 in c.steps) or sorted(c.steps) == list(range(c.count)))
    free = np.array(c.steps) == -1
    assert live[free].all()                                                                    # a term no step owns is never skipped
    if -1 in c.row_last and not free.any():
        b = c.row_last.index(-1)
        assert not live[:, b * c.per:(b + 1) * c.per].any()                                    # a sample with no live term
    if c.nsamples > 1:
        assert -1 in c.row_last and c.count // 2 in c.row_last and max(c.row_last) > max(c.steps)
    terms = R.rows_data(c)
    if c.kind == "lattice":
        assert R.lattice_span(terms) <= 2.0 ** 24
    if not live.all():                                                                         # reading ONE dead word makes the result NaN
        k, j = np.argwhere(~live)[0]
        poisoned = [np.where(live[i], t, np.nan).astype(F64) for i, t in enumerate(terms)]
        clean, _ = R.f64_sum([np.where(live[i], p, 0.0) for i, p in enumerate(poisoned)])
        assert np.isfinite(clean).all()
        leak = [np.where(live[i], p, 0.0) for i, p in enumerate(poisoned)]
        leak[k][j] = poisoned[k][j]
        assert np.isnan(R.f64_sum(leak)[0][j])


def test_row_last_families():
    for ns in (1, 3, 5):
        for k in (5, 32):
            held = {v for rl in R.row_lasts(ns, k) for v in rl}
            assert {-1, k // 2, k + 3} <= held


# ---- column sums -----------------------------------------------------------------------------------------------------------------------------------
def test_pick_G_gives_the_intended_slab_count():
    for c in R.colsum_cases():
        if c.M <= R.COLSUM_SMALL_M:
            assert c.G is None and R.colsum_path(c.M) == "one-launch"
        else:
            assert R.pick_G(c.M, c.C) == c.G and R.colsum_path(c.M) == "two-stage", c.name
    assert {1, 3, 4, 5, 127, 128, 129, 897, 1024, 1025, 3073, 4097, 32769} <= set(R.COLSUM_M) and set(R.COLSUM_C) == {4, 60, 64, 68, 260}
    assert {G for G in R.COLSUM_M.values() if G} >= {8, 24, 25, 32, 33, 256}                   # the second stage's edges: 8 lanes, rounds of 32 slabs
    M, C = R.COLSUM_WIDE
    assert R.pick_G(M, C) == 32 == P.cdiv(2048, P.cdiv(C, 64)) < P.cdiv(M, 128)
    assert {(d, b) for d, b, _ in R.COLSUM_VARIANTS} == {(0, 0), (0, 1), (12, 0), (12, 1)} and {o for _, _, o in R.COLSUM_VARIANTS} == {0, 4}


@pytest.mark.parametrize("c", [c for c in R.colsum_cases() if c.M * c.C < 10 ** 7], ids=lambda c: c.name)
def test_colsum_data(c):
    x, old = R.colsum_data(c)
    assert x.shape == (c.M, c.C) and x.dtype == F32 and old.shape == (c.C,)
    if c.kind == "lattice":
        assert (np.abs(x.astype(F64)).sum(0) + np.abs(old)).max() / 2.0 ** R.COLSUM_UNIT_EXP[0] <= 2.0 ** 24
    else:
        _check_terms(list(x), c.kind, c.name)
    for beta in (0, 1):
        ref, Sp, s, S = R.colsum_ref(x, old, beta)
        got = (old * F32(beta) + s.astype(F32)).astype(F32)                                     # the kernel's two roundings meet the bar
        assert _ratio(got, ref, Sp) <= 1.0
        if c.kind in ("lattice", "wide"):
            assert np.array_equal(got.astype(F64), ref)


def test_largest_lattice_column_sum_stays_inside_24_bits():
    assert 6 * max(R.COLSUM_M) + 3 <= 2 ** 24 and 6 * R.COLSUM_WIDE[0] <= 2 ** 24


# ---- layout, add, ReLU gradient --------------------------------------------------------------------------------------------------------------------
def test_layout_and_relu_restatements():
    for N, C, H, W, Cp in R.NHWC_CASES[:-1]:
        x = R.rng("nhwc").standard_normal((N, C, H, W)).astype(F32)
        y = torch.zeros(N, H, W, Cp)
        y[..., :C] = torch.from_numpy(x).permute(0, 2, 3, 1)
        assert np.array_equal(R.nhwc_ref(x, Cp).view(np.int32), y.numpy().view(np.int32))
    for rows, Cin, Cout in R.PAD_CASES[:-1]:
        x = R.rng("pad").standard_normal((rows, Cin)).astype(F32)
        y = torch.nn.functional.pad(torch.from_numpy(x), (0, Cout - Cin))
        assert np.array_equal(R.pad_ref(x, Cout).view(np.int32), y.numpy().view(np.int32))
    for n in R.RELU_N[:-1]:
        dy, y = R.relu_data(n)
        ref = R.relu_ref(dy, y)
        assert np.isfinite(ref[~(y > 0)]).all() and not ref[~(y > 0)].view(np.int32).any()      # +0 bit for bit, whatever dy holds there
        assert np.array_equal(ref[y > 0].view(np.int32), dy[y > 0].view(np.int32))
        if n >= 255:
            assert {0.0} <= set(y[::3][:7].tolist()) and np.isnan(y).any() and np.signbit(y[y == 0]).any() and (y < 0).any()
            bad = ~(y > 0) & ~np.isfinite(dy)
            assert bad.any() and np.isnan(dy[bad]).any() and np.isinf(dy[bad]).any()
            with np.errstate(invalid="ignore"):
                prod = dy * (y > 0)                                                             # the product form would NOT give zeros there
            assert np.isnan(prod[bad]).all()
