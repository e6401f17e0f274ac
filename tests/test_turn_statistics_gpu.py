"""Turn statistics on the device against the plain-loop restatement tests/turn_statistics_ref.py: the counts of
scanpaths that exist exactly (integers), the closed-form expectation bit for bit (NaN equal to NaN) and, independently of any summation
order, within 1e-12 relative of the exact value; the closed form against the sampler's own kernel over all action sequences; the keyed
functions, the table and the loop."""
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import turn_statistics_ref as R

pytestmark = pytest.mark.gpu
MAPS = {(1, 1): (75.0, 100.0), (1, 3): (75.0, 100.0), (2, 2): (75.0, 100.0), (7, 9): (100.0, 300.0), (30, 40): (240.0, 320.0),
        (32, 64): (256.0, 512.0)}                                       # (7, 9) on 100 x 300: cells that are not square
_ROWS = {}


def M():
    from scanpaths_amd.utils.evaltools import turn_statistics
    return turn_statistics


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(-1)) if got.dtype.kind == "f" \
        else np.flatnonzero((got != want).reshape(-1))
    assert not len(bad), (what, len(bad), bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])


# ---- turn_counts --------------------------------------------------------------------------------------------------------------------------
def count_paths(frame, seed=1):
    """lengths 0, 1, 2, 3, 63, 64 off the pixel grid, fixations on the frame's edges, non-finite coordinates at the start, in the middle
    and at the end"""
    fh, fw = frame
    g = np.random.default_rng(seed)
    nan, inf = float("nan"), float("inf")

    def path(n):
        return np.stack([g.uniform(-0.02 * fw, 1.02 * fw, n), g.uniform(-0.02 * fh, 1.02 * fh, n)], 1)

    paths = [path(n) for n in (0, 1, 2, 3, 63, 64, 7, 9)]
    edges = np.array([(0.0, 0.0), (fw, 1.0), (1.0, 1.0), (1.0, fh), (np.nextafter(fw, 0), np.nextafter(fh, 0)), (0.0, fh / 2), (-0.0, 0.0),
                      (fw / 2, 0.0), (np.nextafter(0.0, -1), 1.0), (fw / 3, fh / 3)])
    paths.append(edges)
    for where, value in ((0, nan), (4, inf), (5, -inf), (8, nan)):
        p = path(9) % np.array([fw, fh])                                 # all inside, so that only the non-finite one drops
        p[where, where % 2] = value
        paths.append(p)
    return paths


@pytest.mark.parametrize("max_steps", [1, 2, 3, 6, 1000])
@pytest.mark.parametrize("shape,n", [((1, 1), 1), ((1, 3), 2), ((7, 9), 16), ((30, 40), 8)])
def test_turn_counts_equal_the_restatement(shape, n, max_steps):
    frame = MAPS[shape]
    paths = count_paths(frame)
    groups = [k % 3 if k % 3 < 2 else 3 for k in range(len(paths))]     # group 2 of 4 stays empty
    sector = M().turn_sectors(shape, frame, n)
    got = M().turn_counts(paths, groups, 4, frame, shape, max_steps=max_steps, n_directions=n)
    want = R.turn_counts(paths, groups, 4, frame, shape, max_steps, sector)
    for k in ("counts", "pairs", "dropped"):
        same(got[k], want[k], (k, shape, max_steps))
    assert not got["counts"][2].any() and got["counts"].sum() == want["pairs"].sum()
    assert got["pairs"][:3].tolist() == [0, 0, 0] and got["pairs"][3] <= int(max_steps >= 3)      # 0, 1, 2 fixations: no pair; 3: at most one
    if max_steps == 1000:
        # nine fixations hold seven pairs; a dropped one at the start or at the end removes one, one in the middle THREE, not one
        assert got["dropped"][-4:].tolist() == [1, 1, 1, 1] and got["pairs"][-4:].tolist() == [6, 4, 4, 6]
        assert got["pairs"][4] <= 61 and got["pairs"][5] <= 62 and got["pairs"][5] > 0
    if shape == (1, 1):
        assert got["counts"][:, :n, :].sum() == 0 and got["counts"][:, :, :n].sum() == 0       # one cell: every saccade stays


@pytest.mark.parametrize("S", [1, 4, 5])
def test_turn_counts_blocks_with_idle_waves(S):
    frame, shape, n = MAPS[(7, 9)], (7, 9), 8
    paths = count_paths(frame, seed=2)[3:3 + S]
    sector = M().turn_sectors(shape, frame, n)
    got = M().turn_counts(paths, [0] * S, 1, frame, shape, max_steps=64, n_directions=n)
    want = R.turn_counts(paths, [0] * S, 1, frame, shape, 64, sector)
    for k in got:
        same(got[k], want[k], (k, S))
    again = M().turn_counts(paths, [0] * S, 1, frame, shape, max_steps=64, n_directions=n)   # the launcher zeroes the table every time
    same(again["counts"], want["counts"], "second call")


def prologue_paths(frame):
    """lengths 0, 1, 2, 3, 9 and 64 with every fixation inside the frame, then the 9 and the 64 again with one fixation out of the frame
    or NaN at the start, in the middle and at the end"""
    fh, fw = frame
    g = np.random.default_rng(7)

    def inside(n):
        return np.stack([g.uniform(0.0, fw, n), g.uniform(0.0, fh, n)], 1) % np.array([fw, fh])

    paths = [inside(n) for n in (0, 1, 2, 3, 9, 64)]
    for n in (9, 64):
        for where in (0, n // 2, n - 1):
            for value in (float("nan"), -1.0, 2.0 * fw):
                p = inside(n)
                p[where, 0] = value
                paths.append(p)
    return paths


@pytest.mark.parametrize("max_steps", [1, 2, 3, 1000])
@pytest.mark.parametrize("shape", [(1, 1), (1, 3), (7, 9)])
def test_turn_and_saccade_counts_share_one_prologue(shape, max_steps):
    """what scan_lane_cell makes structural: the two counts kernels drop the same fixations, and a scanpath that drops none has one
    pair fewer than saccades (tests/saccade_statistics_ref.py and tests/turn_statistics_ref.py satisfy both on these inputs)"""
    from scanpaths_amd.utils.evaltools import saccade_statistics
    frame = MAPS[shape]
    paths = prologue_paths(frame)
    groups = [k % 2 for k in range(len(paths))]
    sacc = saccade_statistics.saccade_counts(paths, groups, 2, frame, shape, max_steps=max_steps)
    turn = M().turn_counts(paths, groups, 2, frame, shape, max_steps=max_steps, n_directions=4)
    same(turn["dropped"], sacc["dropped"], ("dropped", shape, max_steps))
    clean = sacc["dropped"] == 0
    assert clean[:6].all() and (max_steps < 9 or not clean[6:].any())                  # both kinds of scanpath are among the inputs
    same(turn["pairs"][clean], np.maximum(sacc["saccades"][clean] - 1, 0), ("pairs", shape, max_steps))


def test_turn_counts_guards_itself_at_the_c_entry_point():
    """a count the kernel cannot hold or a group that does not exist (the Python layer refuses both earlier): -1, nothing read or
    counted; a sector-table entry outside [0, n] is read as n (what such a table counts is unspecified, the access stays in bounds)"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import _batch
    L = hip.lib()
    n = 4
    rows = np.array([[1.0, 1.0], [12.0, 2.0], [3.0, 23.0], [3.0, 23.0]])
    counts = np.array([65, 3, -1, 4, 3, 3], dtype=np.int32)
    starts = np.array([0, 0, 0, 0, 1, 0], dtype=np.int64)               # (rows that would count, were they read)
    group = np.array([0, 1, 0, 0, 2, -1], dtype=np.int32)
    sector = R.sectors((3, 4), (30.0, 40.0), n)
    sector[4, 2] = 99                                                    # (+2, -1): the second saccade below
    broken = np.where(sector > n, n, sector)
    buf, at = _batch.upload(dict(rows=rows, starts=starts, counts=counts, group=group, sector=sector), dev())
    out = _batch.Out({"counts": (np.int64, 2 * 25), "pairs": (np.int32, 6), "dropped": (np.int32, 6)}, dev())
    hip.check(L.sp_scan_turn_counts(at["rows"], 2, at["starts"], at["counts"], at["group"], 6, 2, 6, 3, 4, 40.0, 30.0, at["sector"], n,
                                    out.ptr("counts"), out.ptr("pairs"), out.ptr("dropped"), hip.stream()), "sp_scan_turn_counts")
    host = out.host()
    assert host["pairs"].tolist() == [-1, 1, -1, 2, -1, -1] and host["dropped"].tolist() == [0] * 6
    want = R.turn_counts([rows[:3], rows[:4]], [1, 0], 2, (30.0, 40.0), (3, 4), 6, broken)["counts"]
    assert want[1, 0, n] == 1 and want[0, 0, n] == 1 and want[0, n, n] == 1 and want.sum() == 3
    same(host["counts"].reshape(2, 5, 5), want, "counts")


# ---- turn_expectation ---------------------------------------------------------------------------------------------------------------------
def expect_case(shape, T):
    """raw positive float32 rows, not normalised, with p_0 <= Z at every step: 0 good, 1 a zero step at t = 1, 2 good, 3 a NaN cell at
    t = 0, 4 an inf cell at the last step, 5 a zero step at t = 3 only (bad only when Tm > 3: with Tm = 3 the one triple counts and the
    zero step beyond Tm is never read), 6 good (its group does not exist where the test says so)"""
    key = (shape, T)
    if key not in _ROWS:
        P = shape[0] * shape[1]
        g = np.random.default_rng(100 * P + T)
        probs = g.uniform(0.01, 1.0, (7, T, 1 + P)).astype(np.float32)
        probs[:, :, 0] = (g.uniform(0.05, 0.9, (7, T)) * probs[:, :, 1:].min(2) * P).astype(np.float32)       # p_0 <= Z
        if T > 1:
            probs[1, 1, :] = 0.0
        probs[3, 0, 1 + P // 2] = float("nan")
        probs[4, T - 1, P] = float("inf")
        if T > 3:
            probs[5, 3, :] = 0.0
        _ROWS[key] = (probs, {})
    return _ROWS[key]


def expect_reference(shape, T, n, min_length, max_steps):
    """the restatement's per-row results, computed once per (case, n, min_length, Tm) and shared"""
    probs, cache = expect_case(shape, T)
    key = (n, min_length, min(T, max_steps))
    if key not in cache:
        sector = M().turn_sectors(shape, MAPS[shape], n)
        cache[key] = R.turn_expectation(probs, [0] * len(probs), 1, sector, min_length, max_steps)["rows"]
    return probs, cache[key]


# the smallest shapes at which each branch can go wrong: one cell (stay only), P below, at and above one batch of 256 middle cells and
# no multiple of it, (n + 1)^2 above 256 (two entries per thread), T below, at and above 3, the 2048-cell limit
EXPECT = [((1, 1), 1, 1), ((1, 1), 4, 16), ((1, 3), 2, 2), ((1, 3), 17, 3), ((2, 2), 3, 3), ((2, 2), 16, 8), ((7, 9), 4, 16), ((7, 9), 17, 8),
          ((30, 40), 3, 8), ((30, 40), 16, 8), ((32, 64), 3, 16)]
BIG = {((30, 40), 3): ((0, 1000), (2, 2), (4, 6), (2, 1)), ((30, 40), 16): ((2, 1000), (0, 6), (17, 3)),
       ((32, 64), 3): ((0, 1000), (2, 3), (4, 2))}


@pytest.mark.parametrize("shape,T,n", EXPECT)
def test_turn_expectation_bit_for_bit(shape, T, n):
    frame = MAPS[shape]
    combos = BIG.get((shape, T)) or [(ml, ms) for ml in (0, 2, T + 1) for ms in (1, 2, 3, 6, 1000)]
    for min_length, max_steps in combos:                                 # the large maps: every value once, not every pair
        probs, rows = expect_reference(shape, T, n, min_length, max_steps)
        sector = M().turn_sectors(shape, frame, n)
        dp = torch.from_numpy(probs).to(dev())
        for R_, groups, G in ((7, [0, 1, 0, 3, 0, 1, 0], 4), (1, [0], 1), (4, [1, 1, 0, 0], 2), (5, [0, 2, 0, 2, 0], 3)):
            # G = 4: group 2 is empty, group 3 holds only the NaN row; R = 5, G = 3: group 2 holds only bad rows (when Tm > 1)
            got = M().turn_expectation(dp[:R_], groups, G, min_length=min_length, max_steps=max_steps, frame_size=frame, n_directions=n,
                                       map_shape=shape)
            want = R.turn_expectation(probs[:R_], groups, G, sector, min_length, max_steps, rows=rows[:R_])
            for k in ("M", "pairs", "bad"):
                same(got[k], want[k], (k, shape, T, min_length, max_steps, R_))
            Tm = min(T, max_steps)
            bad = [0, int(Tm > 1), 0, 1, int(Tm == T), int(Tm > 3), 0][:R_]
            assert got["bad"].tolist() == bad and np.isnan(got["pairs"]).tolist() == [b == 1 for b in bad]
            if Tm < 3:
                assert not got["M"].any() and (got["pairs"][np.array(bad) == 0] == 0).all()
            else:
                assert got["M"][0].sum() > 0
            if G == 4:
                assert not got["M"][2].any() and not got["M"][3].any()
            if shape == (1, 1):
                assert not got["M"][:, :n, :].any() and not got["M"][:, :, :n].any()         # one cell: every saccade stays


def test_turn_expectation_guards_itself_at_the_c_entry_point():
    """a row_group outside [0, ngroups) (the Python layer refuses it earlier): bad -1, NaN, nothing of the row is read or added; a
    sector-table entry outside [0, n] is read as n"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import _batch
    shape, T, n = (7, 9), 4, 8
    probs, _ = expect_case(shape, T)
    L = hip.lib()
    groups = np.array([0, 5, -1, 1, 2, 0, 1], dtype=np.int32)
    sector = M().turn_sectors(shape, MAPS[shape], n)
    sector[0, 0], sector[12, 3] = -7, 1 << 20
    broken = np.where((sector < 0) | (sector > n), n, sector).astype(np.int32)
    E = (n + 1) ** 2
    buf, at = _batch.upload({"row_group": groups, "sector": sector}, dev())
    dp = torch.from_numpy(probs).to(dev())
    work = torch.empty(7 * 2 * E, dtype=torch.float64, device=dev())
    out = _batch.Out({"M": (np.float64, 2 * E), "pairs": (np.float64, 7), "bad": (np.int32, 7)}, dev())
    hip.check(L.sp_scan_turn_expectation(hip.ptr(dp), at["row_group"], 7, T, 7, 9, 2, 1, 1000, at["sector"], n, hip.ptr(work), out.ptr("M"),
                                         out.ptr("pairs"), out.ptr("bad"), hip.stream()), "sp_scan_turn_expectation")
    host = out.host()
    want = R.turn_expectation(probs, groups, 2, broken, 1, 1000)
    assert want["bad"].tolist() == [0, -1, -1, 1, -1, 1, 0]                          # row 5: its zero step t = 3 is inside Tm = 4
    for k in ("pairs", "bad"):
        same(host[k], want[k], k)
    same(host["M"].reshape(2, n + 1, n + 1), want["M"], "M")


def test_turn_expectation_keeps_probs_on_the_device_and_reads_any_float_dtype():
    shape, T, n = (7, 9), 4, 16
    frame = MAPS[shape]
    probs, rows = expect_reference(shape, T, n, 0, 1000)
    dp = torch.from_numpy(probs[[0, 2]]).to(dev())
    want = R.turn_expectation(probs[[0, 2]], [0, 0], 1, M().turn_sectors(shape, frame, n), 0, 1000, rows=[rows[0], rows[2]])
    kw = dict(min_length=0, max_steps=1000, frame_size=frame, n_directions=n)
    for tensor in (dp, dp.double(), dp.expand(2, T, 64).transpose(0, 1).contiguous().transpose(0, 1)):
        same(M().turn_expectation(tensor, [0, 0], 1, map_shape=shape, **kw)["M"], want["M"], str(tensor.dtype))
    with pytest.raises(ValueError, match="map_shape is required"):
        M().turn_expectation(dp, [0, 0], 1, **kw)
    p1201 = torch.rand(1, 3, 1201, device=dev())
    assert M().turn_expectation(p1201, [0], 1, **dict(kw, frame_size=(240, 320)))["M"].shape == (1, 17, 17)      # the one default


@pytest.mark.parametrize("shape,T,n,min_length", [((1, 3), 17, 2, 2), ((2, 2), 16, 8, 0), ((7, 9), 4, 16, 1), ((30, 40), 3, 8, 2),
                                                  ((30, 40), 16, 8, 2), ((32, 64), 3, 8, 0)])
def test_turn_expectation_whatever_the_order_of_the_sums(shape, T, n, min_length):
    """Every M_r entry within 1e-12 RELATIVE of the exactly added exact products of the doubles the kernel multiplies (doubles=True)
    and, beyond that, of the closed form's exact value from the float32 inputs, whatever the order of the Z sums -- rationals for the
    small maps, numpy's extended precision (64 significant bits, summed in another order) for the large ones -- and pairs[r] within
    1e-12 of the table's total.
    The bound counts the roundings of non-negative terms on the longest chain: per map D_t has P / 64 + 8 roundings, at most P per fan,
    at most P over b, T over t and a few products: 2 P + T (P / 64 + 10) + 3 (P / 64 + 8) + T + 8, about 4,900 roundings or 5.5e-13 at
    P = 2048 and T = 16.  Condition: the inputs keep p_0 <= Z at every step (expect_case), so 1 - q_t >= 1/2 and that subtraction
    cannot amplify.  The large maps take two rows (the 16-step one a single row and the float32 inputs only): their wide reference is
    what takes the time."""
    probs, _ = expect_case(shape, T)
    assert (probs[[0, 2, 6], :, 0] <= probs[[0, 2, 6], :, 1:].astype(np.float64).sum(2)).all()
    frame = MAPS[shape]
    sector = M().turn_sectors(shape, frame, n)
    small = shape[0] * shape[1] <= 64
    good = [0, 2, 6] if small else [0, 2] if T < 16 else [2]
    exact = R.row_expectation_exact if small else R.row_expectation_wide
    if not small:
        assert np.finfo(np.longdouble).nmant >= 63, "numpy's long double is no wider than double on this machine"
    for r in good:
        res = M().turn_expectation(torch.from_numpy(probs[[r]]).to(dev()), [0], 1, min_length=min_length, max_steps=1000, frame_size=frame,
                                   n_directions=n, map_shape=shape)
        assert res["bad"].tolist() == [0]
        for doubles in (True, False) if T < 16 or small else (False,):
            Mr, total = exact(probs[r], sector, min_length, 1000, doubles=doubles)
            err = np.abs(res["M"][0] - Mr)
            print(shape, T, r, doubles, "worst relative error", float((err / np.maximum(Mr, 1e-300)).max()))
            assert (err <= 1e-12 * Mr).all(), (r, doubles, float((err / np.maximum(Mr, 1e-300)).max()))
        assert abs(res["pairs"][0] - total) <= 1e-12 * max(total, 1.0)
        assert abs(res["pairs"][0] - math.fsum(res["M"].reshape(-1).tolist())) <= 1e-12 * max(total, 1.0)


# ---- the closed form against the sampler's own kernel ------------------------------------------------------------------------------------
def test_sampled_and_exact_forms_agree_over_all_sequences():
    """all 5^4 action sequences of a T = 4, 2 x 2 case on 75 x 100 go through Sampling.generate_scanpath and turn_counts (one group per
    sequence); weighted by their exact probabilities they give the closed form to 1e-12"""
    from scanpaths_amd.models.sampling import Sampling
    T, Hm, Wm, min_length, n = 4, 2, 2, 1, 4
    frame = (75.0, 100.0)
    g = np.random.default_rng(31)
    probs = g.uniform(0.05, 1.0, (2, T, 5)).astype(np.float32)
    seqs = np.array(list(itertools.product(range(5), repeat=T)), dtype=np.int64)
    s = Sampling(convLSTM_length=T, min_length=min_length, map_width=Wm, map_height=Hm, width=100, height=75)
    fvs, _, _ = s.generate_scanpath(torch.zeros(1), None, torch.ones(len(seqs), T, device=dev()), torch.from_numpy(seqs).to(dev()))
    paths = [np.stack([fv["start_x"], fv["start_y"]], 1) for fv in fvs]
    counts = M().turn_counts(paths, np.arange(len(seqs)), len(seqs), frame, (Hm, Wm), max_steps=T, n_directions=n)
    assert (counts["dropped"] == 0).all() and counts["counts"].shape == (625, n + 1, n + 1)
    exact = M().turn_expectation(torch.from_numpy(probs).to(dev()), [0, 1], 2, min_length=min_length, max_steps=T, frame_size=frame,
                                 n_directions=n, map_shape=(Hm, Wm))
    sector = R.sectors((Hm, Wm), frame, n)
    for row in range(2):
        table = [[Fraction(0)] * (n + 1) for _ in range(n + 1)]
        total = Fraction(0)
        for k, seq in enumerate(seqs):
            w = Fraction(1)
            for t, a in enumerate(seq):
                allowed = range(1, 5) if t < min_length else range(5)
                w *= Fraction(float(probs[row, t, a])) / sum(Fraction(float(probs[row, t, j])) for j in allowed) if a in allowed else 0
            total += w
            if w and (seq != 0).all():                                   # a sequence without terminate: the pixel falls back into its cell
                want = R.turn_counts([np.array([(((a - 1) % Wm + 0.5) * 50.0, ((a - 1) // Wm + 0.5) * 37.5) for a in seq])], [0], 1,
                                     frame, (Hm, Wm), T, sector)["counts"][0]
                assert np.array_equal(counts["counts"][k], want) and want.sum() == 2, (seq, counts["counts"][k], want)
            for r in range(n + 1):
                for c in range(n + 1):
                    if counts["counts"][k, r, c]:
                        table[r][c] += w * int(counts["counts"][k, r, c])
        assert total == 1
        for r in range(n + 1):
            for c in range(n + 1):
                assert abs(float(table[r][c]) - exact["M"][row, r, c]) <= 1e-12, (row, r, c, float(table[r][c]), exact["M"][row, r, c])
        assert abs(float(sum(sum(v) for v in table)) - exact["pairs"][row]) <= 1e-12


# ---- keyed calls, the table, the loop ----------------------------------------------------------------------------------------------------
EV = dict(frame_size=(240, 320), map_shape=(30, 40), max_steps=6, n_directions=8)


def _keyed_case():
    g = np.random.default_rng(41)
    keys = ["q1", "q2", "q3", "q4"]

    def path():
        n = int(g.integers(0, 9))
        return np.stack([g.uniform(-10, 330, n), g.uniform(-10, 250, n), g.uniform(0.1, 0.5, n)], 1)

    gt_keys = [k for k in keys for _ in range(5)]
    pred_keys = [k for k in keys for _ in range(3)] + ["q1"]
    return keys, [path() for _ in gt_keys], gt_keys, [path() for _ in pred_keys], pred_keys


def _equal(a, b, what):
    assert type(a) is type(b) or (np.isscalar(a) and np.isscalar(b)), (what, type(a), type(b))
    if isinstance(a, dict):
        assert set(a) == set(b), (what, set(a) ^ set(b))
        for k in a:
            _equal(a[k], b[k], (what, k))
    else:
        assert np.array_equal(a, b, equal_nan=True), (what, a, b)


def test_keyed_evaluation_human_row_groups_and_table_merge():
    from scanpaths_amd.utils import evaluation as E
    keys, gt, gt_keys, pred, pred_keys = _keyed_case()
    tasks = {"q1": "cup", "q2": "fork", "q3": "cup", "q4": "fork"}
    sector = M().turn_sectors(EV["map_shape"], EV["frame_size"], 8)
    means, per_key = E.turn_statistics_evaluation(gt, pred, gt_keys, pred_keys, groups=tasks, **EV)
    assert per_key["keys"] == keys and set(means["by_group"]) == {"cup", "fork"}
    for prefix, paths, pk in (("", pred, pred_keys), ("human_", gt, gt_keys)):
        res = R.turn_counts([p[:, :2] for p in paths], [0] * len(paths), 1, EV["frame_size"], EV["map_shape"], 6, sector)
        same(means[prefix + "table_sum"], res["counts"][0], prefix + "table")
        assert means[prefix + "pairs_sum"] == res["pairs"].sum() == means[prefix + "table_sum"].sum() > 0
        assert means[prefix + "fixations_dropped"] == res["dropped"].sum() > 0 and means[prefix + "scanpaths_count"] == len(paths)
        _equal(means[prefix + "summary"], M().turn_summary(res["counts"][0]), prefix + "summary")
        for q, k in enumerate(keys):
            mine = np.array([kk == k for kk in pk])
            assert per_key[prefix + "pairs"][q] == res["pairs"][mine].sum() and per_key[prefix + "dropped"][q] == res["dropped"][mine].sum()
        for task in ("cup", "fork"):
            mine = [i for i, k in enumerate(pk) if tasks[k] == task]
            part = R.turn_counts([paths[i][:, :2] for i in mine], [0] * len(mine), 1, EV["frame_size"], EV["map_shape"], 6, sector)
            same(means["by_group"][task][prefix + "table_sum"], part["counts"][0], (prefix, task))
        same(sum(means["by_group"][task][prefix + "table_sum"] for task in ("cup", "fork")), means[prefix + "table_sum"], "groups sum")
    want = M().turn_comparison(means["table_sum"], means["human_table_sum"])
    assert set(want) == {"JSD_turn", "JSD_transition"} and all(means[k] == v and 0 <= v <= 1 for k, v in want.items())
    assert set(want) <= set(means["by_group"]["cup"])
    assert not any(isinstance(v, np.ndarray) and v.ndim > 1 for v in per_key.values())      # no table per key
    # the human-only call equals the human half of the full call
    human, human_keys = E.turn_statistics_human_evaluation(gt, gt_keys, groups=tasks, **EV)
    assert set(human) == {k for k in means if k.startswith("human_")} | {"by_group"}
    for k, v in human.items():
        if k != "by_group":
            _equal(v, means[k], k)
    for task, part in human["by_group"].items():
        _equal(part, {k: v for k, v in means["by_group"][task].items() if k.startswith("human_")}, task)
    assert np.array_equal(human_keys["human_pairs"], per_key["human_pairs"])
    # two batches merged by the table equal one call on their union, exactly: every merged entry is an integer
    table = E.TurnStatisticsTable(EV["n_directions"])
    for part in (("q1", "q2"), ("q3", "q4")):
        gi, pi = [i for i, k in enumerate(gt_keys) if k in part], [i for i, k in enumerate(pred_keys) if k in part]
        table.add(E.turn_statistics_evaluation([gt[i] for i in gi], [pred[i] for i in pi], [gt_keys[i] for i in gi],
                                               [pred_keys[i] for i in pi], groups=tasks, **EV)[0])
    _equal(table.result(), means, "table")
    pooled, _ = E.turn_statistics_evaluation(gt, pred, gt_keys, pred_keys, **EV)             # the default: one pooled group
    _equal(pooled, {k: v for k, v in means.items() if k != "by_group"}, "pooled")


def test_model_evaluation_heads_groups_and_table(monkeypatch):
    from scanpaths_amd.utils import evaluation as E
    g = np.random.default_rng(51)
    N, T, shape, frame, n = 4, 5, (6, 8), (48, 64), 4
    A = 1 + shape[0] * shape[1]
    mk = lambda: g.dirichlet(np.ones(A), (N, T)).astype(np.float32)                         # noqa: E731
    host = {"all_actions_prob": mk(), "good_all_actions_prob": mk(), "poor_all_actions_prob": mk()}
    host["all_actions_prob"][3, 1, 1:] = 0.0                                                # sample 3: a step without cell mass,
    predict = {k: torch.from_numpy(v).to(dev()) for k, v in host.items()}
    keys = ["a", "b", "a", "c"]
    performances = [[True, False, True], [False], [], [True, True]]
    kw = dict(min_length=2, max_steps=4, n_directions=n, frame_size=frame, map_shape=shape)  # bad, as terminate is masked at t = 1
    sector = M().turn_sectors(shape, frame, n)
    # one head
    means, per_key = E.turn_statistics_model_evaluation(predict, keys, **kw)
    want = R.turn_expectation(host["all_actions_prob"], [0] * N, 1, sector, 2, 4)
    same(means["table_sum"], want["M"][0], "table_sum")
    assert want["bad"].tolist() == [0, 0, 0, 1] and means["rows_count"] == 3 and means["rows_bad"] == 1 and per_key["keys"] == ["a", "b", "c"]
    assert means["pairs_sum"] == float(want["pairs"][:3].sum()) and set(means) == {"table_sum", "pairs_sum", "rows_count", "rows_bad", "summary"}
    same(per_key["pairs"], np.array([(want["pairs"][0] + want["pairs"][2]) / 2, want["pairs"][1], np.nan]), "per key")
    _equal(means["summary"], M().turn_summary(means["table_sum"]), "summary")
    human = g.integers(0, 9, (n + 1, n + 1))
    full = E.turn_statistics_model_evaluation(predict, keys, human_table=human, groups={"a": 0, "b": 1, "c": 0}, **kw)[0]
    assert all(full[k] == v for k, v in M().turn_comparison(full["table_sum"], human).items())
    by = R.turn_expectation(host["all_actions_prob"], [0, 1, 0, 0], 2, sector, 2, 4, rows=want["rows"])
    same(full["by_group"][0]["table_sum"], by["M"][0], "label 0")
    same(full["by_group"][1]["table_sum"], by["M"][1], "label 1")
    assert full["by_group"][0]["rows_bad"] == 1 and full["by_group"][1]["rows_count"] == 1 and "JSD_turn" not in full["by_group"][0]
    same(full["by_group"][0]["table_sum"] + full["by_group"][1]["table_sum"], full["table_sum"], "the groups' tables sum to the pooled one")
    assert np.allclose(full["table_sum"], means["table_sum"], rtol=4 * 2.0 ** -53, atol=0)              # (M_0 + M_2) + M_1 against row order
    # the two AiR heads: the rows are the ones saccade_statistics_model_evaluation reads for the same performances
    seen = {}
    real = M().turn_expectation

    def spy(probs, row_groups, n_groups, **k):
        seen["probs"] = probs.cpu().numpy()
        return real(probs, row_groups, n_groups, **k)

    monkeypatch.setattr(M(), "turn_expectation", spy)
    means2, per_key2 = E.turn_statistics_model_evaluation(predict, keys, performances=performances, **kw)
    both = np.concatenate([host["good_all_actions_prob"], host["poor_all_actions_prob"]], 0)
    rows = [0, N + 0, 0, N + 1, 3, 3]                                                       # built by hand from performances
    assert np.array_equal(seen["probs"], both[rows])
    want2 = R.turn_expectation(both[rows], [0] * 6, 1, sector, 2, 4)
    same(means2["table_sum"], want2["M"][0], "two heads")
    assert means2["rows_count"] == 6 and means2["rows_bad"] == 0 and np.isnan(per_key2["pairs"]).tolist() == [False, False, False]
    # the table over two batches equals one call on their union to rounding: both are sums of the same N <= 4 non-negative M_r per
    # entry in two associations, each within N * 2^-53 relative of the true sum
    table = E.TurnStatisticsTable(n)
    for lo in (0, 2):
        sl = {k: v[lo:lo + 2] for k, v in predict.items()}
        table.add(E.turn_statistics_model_evaluation(sl, keys[lo:lo + 2], **kw)[0])
    merged = table.result(human)
    assert merged["rows_count"] == 3 and merged["rows_bad"] == 1
    assert np.allclose(merged["table_sum"], means["table_sum"], rtol=1e-13, atol=0)
    assert abs(merged["pairs_sum"] - means["pairs_sum"]) <= 1e-13 * means["pairs_sum"]
    assert merged["JSD_turn"] == M().turn_comparison(merged["table_sum"], human)["JSD_turn"] and abs(merged["JSD_turn"] - full["JSD_turn"]) <= 1e-12


def test_turn_statistics_loop_on_a_tiny_multihead_model(monkeypatch):
    from scanpaths_amd import hip, inference
    from scanpaths_amd.models.baseline_attention_multihead import baseline
    from scanpaths_amd.procedural import fill_module
    from scanpaths_amd.synth import make_batch
    from scanpaths_amd.utils import evaluation as E
    T, B, n = 3, 2, 8
    batches = [make_batch("COCO_Search18", B, 240, 320, T, seed=9 + k) for k in range(2)]
    model = baseline(convLSTM_length=T)
    fill_module(model, 9, family="tame")
    model = model.to(dev())
    loader = [{"images": b["images"], "attention_maps": b["attention_maps"], "tasks": b["tasks"], "question_ids": [f"s{2 * k}", f"s{2 * k + 1}"]}
              for k, b in enumerate(batches)]
    L = hip.lib()
    launches, launch = [], L.sp_scan_turn_expectation
    monkeypatch.setattr(L, "sp_scan_turn_expectation", lambda *a: launches.append(1) or launch(*a))
    for name in ("sp_sample_actions", "sp_generate_scanpath", "sp_beam_search"):
        monkeypatch.setattr(L, name, lambda *a: (_ for _ in ()).throw(AssertionError("the turn-statistics loop does not sample")))
    human = np.random.default_rng(2).integers(0, 5, (n + 1, n + 1))
    means, per_batch = inference.run_turn_statistics_loop(model, loader, min_length=1, max_steps=3, n_directions=n, human_table=human)
    assert len(launches) == 2 and len(per_batch) == 2 and per_batch[1]["keys"] == ["s2", "s3"] and not model.training
    table = E.TurnStatisticsTable(n)
    for k, b in enumerate(batches):
        with torch.no_grad():
            predict = model(b["images"].to(dev()), b["attention_maps"].to(dev()), b["tasks"].to(dev()))
        assert tuple(predict["all_actions_prob"].shape) == (B, T, 1201)
        direct = M().turn_expectation(predict["all_actions_prob"], [0, 0], 1, min_length=1, max_steps=3, frame_size=(240, 320), n_directions=n)
        ev, keyed = E.turn_statistics_model_evaluation(predict, loader[k]["question_ids"], min_length=1, max_steps=3, n_directions=n)
        same(ev["table_sum"], direct["M"][0], "evaluation")
        same(keyed["pairs"], direct["pairs"], "per key")
        same(per_batch[k]["pairs"], direct["pairs"], "loop per key")
        table.add(ev)
    _equal(means, table.result(human), "the loop returns the table of its batches")
    assert means["rows_count"] == 4 and 0 < means["pairs_sum"] <= 4 and 0 <= means["JSD_turn"] <= 1 and 0 <= means["JSD_transition"] <= 1
    assert abs(means["summary"]["total"] - means["pairs_sum"]) <= 1e-12 * means["pairs_sum"]
