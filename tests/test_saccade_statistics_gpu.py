"""Saccade statistics on the device against the plain-loop restatement tests/saccade_statistics_ref.py: the counts of
scanpaths that exist exactly (integers), the closed-form expectation bit for bit (NaN equal to NaN) and, independently of any summation
order, within 1e-12 relative of the exact rational value; the closed form against the sampler's own kernel over all action sequences;
the keyed functions, the table and the loop."""
import itertools
import math
from fractions import Fraction

import numpy as np
import pytest
import torch

import saccade_statistics_ref as R

pytestmark = pytest.mark.gpu
MAPS = {(1, 1): (75.0, 100.0), (1, 3): (75.0, 100.0), (2, 2): (75.0, 100.0), (7, 9): (75.0, 100.0), (30, 40): (240.0, 320.0),
        (32, 64): (256.0, 512.0)}
_ROWS = {}


def M():
    from scanpaths_amd.utils.evaltools import saccade_statistics
    return saccade_statistics


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(-1)) if got.dtype.kind == "f" \
        else np.flatnonzero((got != want).reshape(-1))
    assert not len(bad), (what, len(bad), bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])


# ---- saccade_counts -----------------------------------------------------------------------------------------------------------------------
def count_paths(frame, seed=1):
    """lengths 0, 1, 2, 63, 64 off the pixel grid, fixations on the frame's edges, non-finite coordinates at the start, in the middle
    and at the end"""
    fh, fw = frame
    g = np.random.default_rng(seed)
    nan, inf = float("nan"), float("inf")

    def path(n):
        return np.stack([g.uniform(-0.05 * fw, 1.05 * fw, n), g.uniform(-0.05 * fh, 1.05 * fh, n)], 1)

    paths = [path(n) for n in (0, 1, 2, 63, 64, 7, 9)]
    edges = np.array([(0.0, 0.0), (fw, 1.0), (1.0, 1.0), (1.0, fh), (np.nextafter(fw, 0), np.nextafter(fh, 0)), (0.0, fh / 2), (-0.0, 0.0),
                      (fw / 2, 0.0), (np.nextafter(0.0, -1), 1.0), (fw / 3, fh / 3)])
    paths.append(edges)
    for where, value in ((0, nan), (3, inf), (7, -inf), (8, nan)):
        p = path(9) % np.array([fw, fh])                                 # all inside, so that only the non-finite one drops
        p[where if where < 8 else -1, where % 2] = value
        paths.append(p)
    return paths


@pytest.mark.parametrize("max_steps", [1, 2, 6, 1000])
@pytest.mark.parametrize("shape", [(1, 1), (1, 3), (7, 9), (30, 40)])
def test_saccade_counts_equal_the_restatement(shape, max_steps):
    frame = MAPS[shape]
    paths = count_paths(frame)
    groups = [k % 3 if k % 3 < 2 else 3 for k in range(len(paths))]     # group 2 of 4 stays empty
    got = M().saccade_counts(paths, groups, 4, frame, shape, max_steps=max_steps)
    want = R.saccade_counts(paths, groups, 4, frame, shape, max_steps)
    for k in ("counts", "saccades", "dropped"):
        same(got[k], want[k], (k, shape, max_steps))
    assert not got["counts"][2].any() and got["counts"].sum() == want["saccades"].sum()
    if max_steps == 1000:
        assert got["dropped"][-4:].tolist() == [1, 1, 1, 1] and got["saccades"][-4:].tolist() == [7, 6, 6, 7]     # no bridging
        assert got["dropped"][7] == 3                                    # x = frame_w, y = frame_h and the negative denormal are outside


@pytest.mark.parametrize("S", [1, 4, 5])
def test_saccade_counts_blocks_with_idle_waves(S):
    frame, shape = MAPS[(7, 9)], (7, 9)
    paths = count_paths(frame, seed=2)[2:2 + S]
    got = M().saccade_counts(paths, [0] * S, 1, frame, shape, max_steps=64)
    want = R.saccade_counts(paths, [0] * S, 1, frame, shape, 64)
    for k in got:
        same(got[k], want[k], (k, S))
    again = M().saccade_counts(paths, [0] * S, 1, frame, shape, max_steps=64)               # the launcher zeroes the lattice every time
    same(again["counts"], want["counts"], "second call")


def test_saccade_counts_guards_itself_at_the_c_entry_point():
    """a count the kernel cannot hold or a group that does not exist (the Python layer refuses both earlier): -1, nothing read or counted"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import _batch
    L = hip.lib()
    rows = np.array([[1.0, 1.0], [12.0, 2.0], [3.0, 23.0]])
    counts = np.array([65, 2, -1, 3, 2, 2], dtype=np.int32)
    starts = np.array([0, 0, 0, 0, 1, 0], dtype=np.int64)               # (rows that would count, were they read)
    group = np.array([0, 1, 0, 0, 2, -1], dtype=np.int32)
    buf, at = _batch.upload(dict(rows=rows, starts=starts, counts=counts, group=group), dev())
    out = _batch.Out({"counts": (np.int64, 2 * 5 * 7), "saccades": (np.int32, 6), "dropped": (np.int32, 6)}, dev())
    hip.check(L.sp_scan_saccade_counts(at["rows"], 2, at["starts"], at["counts"], at["group"], 6, 2, 6, 3, 4, 40.0, 30.0, out.ptr("counts"),
                                       out.ptr("saccades"), out.ptr("dropped"), hip.stream()), "sp_scan_saccade_counts")
    host = out.host()
    assert host["saccades"].tolist() == [-1, 1, -1, 2, -1, -1] and host["dropped"].tolist() == [0] * 6
    want = np.zeros((2, 5, 7), np.int64)
    want[1, 2, 4] += 1                                                   # (1, 1) -> (12, 2): one column right
    want[0, 2, 4] += 1
    want[0, 4, 2] += 1                                                   # (12, 2) -> (3, 23): two rows down, one column left
    same(host["counts"].reshape(2, 5, 7), want, "counts")


# ---- saccade_expectation ------------------------------------------------------------------------------------------------------------------
def expect_case(shape, T):
    """raw positive float32 rows, not normalised: 0 good, 1 a zero step at t = 1, 2 good, 3 a NaN cell at t = 0, 4 an inf cell at the last
    step, 5 a zero step at t = 2 only (bad only when Tm > 2), 6 good (its group does not exist where the test says so)"""
    key = (shape, T)
    if key not in _ROWS:
        P = shape[0] * shape[1]
        g = np.random.default_rng(100 * P + T)
        probs = g.uniform(0.01, 1.0, (7, T, 1 + P)).astype(np.float32)
        if T > 1:
            probs[1, 1, 1:] = 0.0
            probs[1, 1, 0] = 0.0
        probs[3, 0, 1 + P // 2] = float("nan")
        probs[4, T - 1, P] = float("inf")
        if T > 2:
            probs[5, 2, :] = 0.0
        _ROWS[key] = (probs, {})
    return _ROWS[key]


def expect_reference(shape, T, min_length, max_steps):
    """the restatement's per-row results, computed once per (case, min_length, Tm) and shared"""
    probs, cache = expect_case(shape, T)
    key = (min_length, min(T, max_steps))
    if key not in cache:
        cache[key] = R.saccade_expectation(probs, [0] * len(probs), 1, shape, min_length, max_steps)["rows"]
    return probs, cache[key]


EXPECT = [((1, 1), 1), ((1, 1), 3), ((1, 3), 2), ((1, 3), 17), ((2, 2), 3), ((2, 2), 16), ((7, 9), 1), ((7, 9), 3), ((7, 9), 17),
          ((30, 40), 2), ((30, 40), 3), ((30, 40), 16), ((32, 64), 2)]


@pytest.mark.parametrize("shape,T", EXPECT)
def test_saccade_expectation_bit_for_bit(shape, T):
    big = shape[0] * shape[1] > 64
    for min_length in (0, 2, T + 1):
        for max_steps in (1, 2, 6, 1000):
            if big and (min_length, max_steps) not in ((0, 1000), (2, 2), (T + 1, 6), (2, 1)):
                continue                                                 # the large maps: every value once, not every pair
            probs, rows = expect_reference(shape, T, min_length, max_steps)
            dp = torch.from_numpy(probs).to(dev())
            for R_, groups, G in ((7, [0, 1, 0, 3, 0, 1, 0], 4), (1, [0], 1), (4, [1, 1, 0, 0], 2), (5, [0, 2, 0, 2, 0], 3)):
                # G = 4: group 2 is empty, group 3 holds only the NaN row; R = 5, G = 3: group 2 holds only bad rows
                got = M().saccade_expectation(dp[:R_], groups, G, min_length=min_length, max_steps=max_steps, map_shape=shape)
                want = R.saccade_expectation(probs[:R_], groups, G, shape, min_length, max_steps, rows=rows[:R_])
                for k in ("E", "saccades", "bad"):
                    same(got[k], want[k], (k, shape, T, min_length, max_steps, R_))
                Tm = min(T, max_steps)
                bad = [0, int(Tm > 1), 0, 1, int(Tm == T), int(Tm > 2), 0][:R_]
                assert got["bad"].tolist() == bad and np.isnan(got["saccades"]).tolist() == [b == 1 for b in bad]
                if Tm < 2:
                    assert not got["E"].any() and (got["saccades"][np.array(bad) == 0] == 0).all()
                if G == 4:
                    assert not got["E"][2].any() and not got["E"][3].any()


def test_saccade_expectation_guards_itself_at_the_c_entry_point():
    """a row_group outside [0, ngroups) (the Python layer refuses it earlier): bad -1, NaN, nothing of the row is read or added"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import _batch
    shape, T = (7, 9), 3
    probs, rows = expect_reference(shape, T, 1, 1000)
    L = hip.lib()
    groups = np.array([0, 5, -1, 1, 2, 0, 1], dtype=np.int32)
    D = 13 * 17
    buf, at = _batch.upload({"row_group": groups}, dev())
    dp = torch.from_numpy(probs).to(dev())
    work = torch.empty(7 * D, dtype=torch.float64, device=dev())
    out = _batch.Out({"E": (np.float64, 2 * D), "saccades": (np.float64, 7), "bad": (np.int32, 7)}, dev())
    hip.check(L.sp_scan_saccade_expectation(hip.ptr(dp), at["row_group"], 7, T, 7, 9, 2, 1, 1000, hip.ptr(work), out.ptr("E"),
                                            out.ptr("saccades"), out.ptr("bad"), hip.stream()), "sp_scan_saccade_expectation")
    host = out.host()
    want = R.saccade_expectation(probs, groups, 2, shape, 1, 1000, rows=rows)
    assert want["bad"].tolist() == [0, -1, -1, 1, -1, 1, 0]                          # row 5: its zero step t = 2 is inside Tm = 3
    for k in ("saccades", "bad"):
        same(host[k], want[k], k)
    same(host["E"].reshape(2, 13, 17), want["E"], "E")


def test_saccade_expectation_keeps_probs_on_the_device_and_reads_any_float_dtype():
    shape, T = (7, 9), 3
    probs, rows = expect_reference(shape, T, 0, 1000)
    dp = torch.from_numpy(probs[[0, 2]]).to(dev())
    want = R.saccade_expectation(probs[[0, 2]], [0, 0], 1, shape, 0, 1000, rows=[rows[0], rows[2]])
    for tensor in (dp, dp.double(), dp.expand(2, T, 64).transpose(0, 1).contiguous().transpose(0, 1)):
        same(M().saccade_expectation(tensor, [0, 0], 1, min_length=0, max_steps=1000, map_shape=shape)["E"], want["E"], str(tensor.dtype))
    with pytest.raises(ValueError, match="map_shape is required"):
        M().saccade_expectation(dp, [0, 0], 1, min_length=0, max_steps=4)
    p1201 = torch.rand(1, 2, 1201, device=dev())
    assert M().saccade_expectation(p1201, [0], 1, min_length=0, max_steps=4)["E"].shape == (1, 59, 79)      # the one default


@pytest.mark.parametrize("shape,T,min_length", [((1, 3), 17, 2), ((2, 2), 16, 0), ((7, 9), 3, 1), ((30, 40), 3, 2), ((32, 64), 2, 0)])
def test_saccade_expectation_whatever_the_order_of_the_sums(shape, T, min_length):
    """Every E_r entry within 1e-12 RELATIVE of the exactly added exact products of the doubles A_t, c_t(i), c_{t+1}(i + d) the kernel
    multiplies (doubles=True) and, beyond that, of the closed form's exact value from the float32 inputs, whatever the order of the Z
    sums -- rationals for the small maps, numpy's extended precision (64 significant bits, summed in another order) for the large
    ones -- and saccades[r] within 1e-12 of the lattice total.
    The bound: an entry is reached through at most 2 P + T + 8 roundings of non-negative terms (the two Z sums, the products' sum, the
    survival recursion, the divisions and products); with P <= 2048 that is 4.6e-13 relative."""
    probs, _ = expect_case(shape, T)
    good = [0, 2, 6]
    got = [M().saccade_expectation(torch.from_numpy(probs[[r]]).to(dev()), [0], 1, min_length=min_length, max_steps=1000, map_shape=shape)
           for r in good]
    exact = R.row_expectation_exact if shape[0] * shape[1] <= 64 else R.row_expectation_wide
    if exact is R.row_expectation_wide:
        assert np.finfo(np.longdouble).nmant >= 63, "numpy's long double is no wider than double on this machine"
    for r, res in zip(good, got):
        assert res["bad"].tolist() == [0]
        for doubles in (True, False):
            E, total = exact(probs[r], shape, min_length, 1000, doubles=doubles)
            err = np.abs(res["E"][0] - E)
            print(shape, T, r, doubles, "worst relative error", float((err / np.maximum(E, 1e-300)).max()))
            assert (err <= 1e-12 * E).all(), (r, doubles, float((err / np.maximum(E, 1e-300)).max()))
        assert abs(res["saccades"][0] - total) <= 1e-12 * max(total, 1.0)
        assert abs(res["saccades"][0] - math.fsum(res["E"].reshape(-1).tolist())) <= 1e-12 * max(total, 1.0)


# ---- the closed form against the sampler's own kernel ------------------------------------------------------------------------------------
def test_sampled_and_exact_forms_agree_over_all_sequences():
    """all 5^3 action sequences of a T = 3, 2 x 2 case on 75 x 100 go through Sampling.generate_scanpath and saccade_counts (one group
    per sequence); weighted by their exact probabilities they give the closed form to 1e-12"""
    from scanpaths_amd.models.sampling import Sampling
    T, Hm, Wm, min_length = 3, 2, 2, 1
    frame = (75.0, 100.0)
    g = np.random.default_rng(31)
    probs = g.uniform(0.05, 1.0, (2, T, 5)).astype(np.float32)
    seqs = np.array(list(itertools.product(range(5), repeat=T)), dtype=np.int64)
    s = Sampling(convLSTM_length=T, min_length=min_length, map_width=Wm, map_height=Hm, width=100, height=75)
    fvs, _, _ = s.generate_scanpath(torch.zeros(1), None, torch.ones(len(seqs), T, device=dev()), torch.from_numpy(seqs).to(dev()))
    paths = [np.stack([fv["start_x"], fv["start_y"]], 1) for fv in fvs]
    counts = M().saccade_counts(paths, np.arange(len(seqs)), len(seqs), frame, (Hm, Wm), max_steps=T)
    assert (counts["dropped"] == 0).all()
    exact = M().saccade_expectation(torch.from_numpy(probs).to(dev()), [0, 1], 2, min_length=min_length, max_steps=T, map_shape=(Hm, Wm))
    for row in range(2):
        lattice = [[Fraction(0)] * 3 for _ in range(3)]
        total = Fraction(0)
        for k, seq in enumerate(seqs):
            w = Fraction(1)
            for t, a in enumerate(seq):
                allowed = range(1, 5) if t < min_length else range(5)
                w *= Fraction(float(probs[row, t, a])) / sum(Fraction(float(probs[row, t, j])) for j in allowed) if a in allowed else 0
            total += w
            if w and (seq != 0).all():                                   # a sequence without terminate: the pixel falls back into its cell
                want = R.saccade_counts([np.array([(((a - 1) % Wm + 0.5) * 50.0, ((a - 1) // Wm + 0.5) * 37.5) for a in seq])], [0], 1,
                                        frame, (Hm, Wm), T)["counts"][0]
                assert np.array_equal(counts["counts"][k], want), (seq, counts["counts"][k], want)
            for r in range(3):
                for c in range(3):
                    lattice[r][c] += w * int(counts["counts"][k, r, c])
        assert total == 1
        for r in range(3):
            for c in range(3):
                assert abs(float(lattice[r][c]) - exact["E"][row, r, c]) <= 1e-12, (row, r, c, float(lattice[r][c]), exact["E"][row, r, c])
        assert abs(float(sum(sum(v) for v in lattice)) - exact["saccades"][row]) <= 1e-12


@pytest.mark.parametrize("shape", list(MAPS))
def test_the_samplers_pixel_falls_back_into_its_cell(shape):
    """every action 1 .. P through Sampling.generate_scanpath, as pairs (cell, next cell): saccade_counts reads the displacement between
    the two cells, for all six map and frame pairs"""
    from scanpaths_amd.models.sampling import Sampling
    Hm, Wm = shape
    fh, fw = MAPS[shape]
    P = Hm * Wm
    nxt = (np.arange(P) * 7 + 3) % P
    actions = torch.from_numpy(np.stack([np.arange(P), nxt], 1) + 1).to(dev())
    s = Sampling(convLSTM_length=2, min_length=2, map_width=Wm, map_height=Hm, width=int(fw), height=int(fh))
    fvs, _, _ = s.generate_scanpath(torch.zeros(1), None, torch.ones(P, 2, device=dev()), actions)
    paths = [np.stack([fv["start_x"], fv["start_y"]], 1) for fv in fvs]
    got = M().saccade_counts(paths, [0] * P, 1, (fh, fw), shape, max_steps=2)
    want = np.zeros((2 * Hm - 1, 2 * Wm - 1), np.int64)
    np.add.at(want, (nxt // Wm - np.arange(P) // Wm + Hm - 1, nxt % Wm - np.arange(P) % Wm + Wm - 1), 1)
    same(got["counts"][0], want, shape)
    assert (got["saccades"] == 1).all() and (got["dropped"] == 0).all()


# ---- keyed calls, the table, the loop ----------------------------------------------------------------------------------------------------
EV = dict(frame_size=(240, 320), map_shape=(30, 40), max_steps=6, amplitude_edges=[0.0, 8.0, 40.0, 120.0, 240.0], n_directions=8)


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
    means, per_key = E.saccade_statistics_evaluation(gt, pred, gt_keys, pred_keys, groups=tasks, **EV)
    assert per_key["keys"] == keys and set(means["by_group"]) == {"cup", "fork"}
    for prefix, paths, pk in (("", pred, pred_keys), ("human_", gt, gt_keys)):
        res = R.saccade_counts([p[:, :2] for p in paths], [0] * len(paths), 1, EV["frame_size"], EV["map_shape"], 6)
        same(means[prefix + "lattice_sum"], res["counts"][0], prefix + "lattice")
        assert means[prefix + "saccades_sum"] == res["saccades"].sum() == means[prefix + "lattice_sum"].sum() > 0
        assert means[prefix + "fixations_dropped"] == res["dropped"].sum() > 0 and means[prefix + "scanpaths_count"] == len(paths)
        _equal(means[prefix + "summary"], M().saccade_summary(res["counts"][0], EV["frame_size"], amplitude_edges=EV["amplitude_edges"],
                                                              n_directions=8), prefix + "summary")
        for q, k in enumerate(keys):
            mine = np.array([kk == k for kk in pk])
            assert per_key[prefix + "saccades"][q] == res["saccades"][mine].sum() and per_key[prefix + "dropped"][q] == res["dropped"][mine].sum()
        for task in ("cup", "fork"):
            mine = [i for i, k in enumerate(pk) if tasks[k] == task]
            part = R.saccade_counts([paths[i][:, :2] for i in mine], [0] * len(mine), 1, EV["frame_size"], EV["map_shape"], 6)
            same(means["by_group"][task][prefix + "lattice_sum"], part["counts"][0], (prefix, task))
    want = M().saccade_comparison(means["lattice_sum"], means["human_lattice_sum"], EV["frame_size"], amplitude_edges=EV["amplitude_edges"],
                                  n_directions=8)
    assert all(means[k] == v and 0 <= v for k, v in want.items()) and set(want) <= set(means["by_group"]["cup"])
    assert not any(isinstance(v, np.ndarray) and v.ndim > 1 for v in per_key.values())      # no lattice per key
    # the human-only call equals the human half of the full call
    human, human_keys = E.saccade_statistics_human_evaluation(gt, gt_keys, groups=tasks, **EV)
    assert set(human) == {k for k in means if k.startswith("human_")} | {"by_group"}
    for k, v in human.items():
        if k != "by_group":
            _equal(v, means[k], k)
    for task, part in human["by_group"].items():
        _equal(part, {k: v for k, v in means["by_group"][task].items() if k.startswith("human_")}, task)
    assert np.array_equal(human_keys["human_saccades"], per_key["human_saccades"])
    # two batches merged by the table equal one call on their union, exactly: every merged entry is an integer
    table = E.SaccadeStatisticsTable(EV["frame_size"], EV["map_shape"], EV["amplitude_edges"], EV["n_directions"])
    for part in (("q1", "q2"), ("q3", "q4")):
        gi, pi = [i for i, k in enumerate(gt_keys) if k in part], [i for i, k in enumerate(pred_keys) if k in part]
        table.add(E.saccade_statistics_evaluation([gt[i] for i in gi], [pred[i] for i in pi], [gt_keys[i] for i in gi],
                                                  [pred_keys[i] for i in pi], groups=tasks, **EV)[0])
    _equal(table.result(), means, "table")
    pooled, _ = E.saccade_statistics_evaluation(gt, pred, gt_keys, pred_keys, **EV)          # the default: one pooled group
    _equal(pooled, {k: v for k, v in means.items() if k != "by_group"}, "pooled")


def test_model_evaluation_heads_groups_and_table(monkeypatch):
    from scanpaths_amd.utils import evaluation as E
    g = np.random.default_rng(51)
    N, T, shape, frame = 4, 5, (6, 8), (48, 64)
    A = 1 + shape[0] * shape[1]
    mk = lambda: g.dirichlet(np.ones(A), (N, T)).astype(np.float32)                         # noqa: E731
    host = {"all_actions_prob": mk(), "good_all_actions_prob": mk(), "poor_all_actions_prob": mk()}
    host["all_actions_prob"][3, 1, 1:] = 0.0                                                # sample 3: a step without cell mass,
    predict = {k: torch.from_numpy(v).to(dev()) for k, v in host.items()}
    keys = ["a", "b", "a", "c"]
    performances = [[True, False, True], [False], [], [True, True]]
    kw = dict(min_length=2, max_steps=4, frame_size=frame, map_shape=shape)                 # bad, as terminate is masked at t = 1
    bins = dict(amplitude_edges=[0.0, 8.0, 24.0, 48.0], n_directions=4)
    # one head
    means, per_key = E.saccade_statistics_model_evaluation(predict, keys, **kw)
    want = R.saccade_expectation(host["all_actions_prob"], [0] * N, 1, shape, 2, 4)
    same(means["lattice_sum"], want["E"][0], "lattice_sum")
    assert want["bad"].tolist() == [0, 0, 0, 1] and means["rows_count"] == 3 and means["rows_bad"] == 1 and per_key["keys"] == ["a", "b", "c"]
    assert means["saccades_sum"] == float(want["saccades"][:3].sum()) and set(means) == {"lattice_sum", "saccades_sum", "rows_count", "rows_bad"}
    same(per_key["saccades"], np.array([(want["saccades"][0] + want["saccades"][2]) / 2, want["saccades"][1], np.nan]), "per key")
    human = g.integers(0, 9, (11, 15))
    full = E.saccade_statistics_model_evaluation(predict, keys, human_lattice=human, groups={"a": 0, "b": 1, "c": 0}, **kw, **bins)[0]
    _equal(full["summary"], M().saccade_summary(full["lattice_sum"], frame, **bins), "summary")
    assert all(full[k] == v for k, v in M().saccade_comparison(full["lattice_sum"], human, frame, **bins).items())
    by = R.saccade_expectation(host["all_actions_prob"], [0, 1, 0, 0], 2, shape, 2, 4, rows=want["rows"])
    same(full["by_group"][0]["lattice_sum"], by["E"][0], "label 0")
    same(full["by_group"][1]["lattice_sum"], by["E"][1], "label 1")
    assert full["by_group"][0]["rows_bad"] == 1 and full["by_group"][1]["rows_count"] == 1 and "JSD_lattice" not in full["by_group"][0]
    assert np.allclose(full["lattice_sum"], means["lattice_sum"], rtol=4 * 2.0 ** -53, atol=0)          # (E_0 + E_2) + E_1 against row order
    # the two AiR heads: the rows are the ones search_efficiency_model_evaluation reads for the same performances
    seen = {}
    real = M().saccade_expectation

    def spy(probs, row_groups, n_groups, **k):
        seen["probs"] = probs.cpu().numpy()
        return real(probs, row_groups, n_groups, **k)

    monkeypatch.setattr(M(), "saccade_expectation", spy)
    means2, per_key2 = E.saccade_statistics_model_evaluation(predict, keys, performances=performances, **kw)
    both = np.concatenate([host["good_all_actions_prob"], host["poor_all_actions_prob"]], 0)
    rows = [0, N + 0, 0, N + 1, 3, 3]                                                       # built by hand from performances
    assert np.array_equal(seen["probs"], both[rows])
    want2 = R.saccade_expectation(both[rows], [0] * 6, 1, shape, 2, 4)
    same(means2["lattice_sum"], want2["E"][0], "two heads")
    assert means2["rows_count"] == 6 and means2["rows_bad"] == 0 and np.isnan(per_key2["saccades"]).tolist() == [False, False, False]
    # the table over two batches equals one call on their union to rounding: both are sums of the same N <= 4 non-negative E_r per
    # entry in two associations, each within N * 2^-53 relative of the true sum
    table = E.SaccadeStatisticsTable(frame, shape, **bins)
    for lo in (0, 2):
        sl = {k: v[lo:lo + 2] for k, v in predict.items()}
        table.add(E.saccade_statistics_model_evaluation(sl, keys[lo:lo + 2], **kw)[0])
    merged = table.result(human)
    assert merged["rows_count"] == 3 and merged["rows_bad"] == 1
    assert np.allclose(merged["lattice_sum"], means["lattice_sum"], rtol=1e-12, atol=0)
    assert abs(merged["saccades_sum"] - means["saccades_sum"]) <= 1e-12 * means["saccades_sum"]
    assert merged["JSD_lattice"] == M().jensen_shannon(merged["lattice_sum"], human) and abs(merged["JSD_lattice"] - full["JSD_lattice"]) <= 1e-12


def test_saccade_statistics_loop_on_a_tiny_multihead_model(monkeypatch):
    from scanpaths_amd import hip, inference
    from scanpaths_amd.models.baseline_attention_multihead import baseline
    from scanpaths_amd.procedural import fill_module
    from scanpaths_amd.synth import make_batch
    from scanpaths_amd.utils import evaluation as E
    T, B = 2, 2
    batches = [make_batch("COCO_Search18", B, 240, 320, T, seed=9 + k) for k in range(2)]
    model = baseline(convLSTM_length=T)
    fill_module(model, 9, family="tame")
    model = model.to(dev())
    loader = [{"images": b["images"], "attention_maps": b["attention_maps"], "tasks": b["tasks"], "question_ids": [f"s{2 * k}", f"s{2 * k + 1}"]}
              for k, b in enumerate(batches)]
    L = hip.lib()
    launches, launch = [], L.sp_scan_saccade_expectation
    monkeypatch.setattr(L, "sp_scan_saccade_expectation", lambda *a: launches.append(1) or launch(*a))
    for name in ("sp_sample_actions", "sp_generate_scanpath", "sp_beam_search"):
        monkeypatch.setattr(L, name, lambda *a: (_ for _ in ()).throw(AssertionError("the saccade-statistics loop does not sample")))
    bins = dict(amplitude_edges=[0.0, 8.0, 80.0, 400.0], n_directions=8)
    human = np.random.default_rng(2).integers(0, 5, (59, 79))
    means, per_batch = inference.run_saccade_statistics_loop(model, loader, min_length=1, max_steps=3, human_lattice=human, **bins)
    assert len(launches) == 2 and len(per_batch) == 2 and per_batch[1]["keys"] == ["s2", "s3"] and not model.training
    table = E.SaccadeStatisticsTable((240, 320), (30, 40), **bins)
    for k, b in enumerate(batches):
        with torch.no_grad():
            predict = model(b["images"].to(dev()), b["attention_maps"].to(dev()), b["tasks"].to(dev()))
        assert tuple(predict["all_actions_prob"].shape) == (B, T, 1201)
        direct = M().saccade_expectation(predict["all_actions_prob"], [0, 0], 1, min_length=1, max_steps=3)
        ev, keyed = E.saccade_statistics_model_evaluation(predict, loader[k]["question_ids"], min_length=1, max_steps=3)
        same(ev["lattice_sum"], direct["E"][0], "evaluation")
        same(keyed["saccades"], direct["saccades"], "per key")
        same(per_batch[k]["saccades"], direct["saccades"], "loop per key")
        table.add(ev)
    _equal(means, table.result(human), "the loop returns the table of its batches")
    assert means["rows_count"] == 4 and 0 < means["saccades_sum"] <= 4 and 0 <= means["JSD_lattice"] <= 1 and means["W1_amplitude"] >= 0
    assert abs(means["summary"]["total"] - means["saccades_sum"]) <= 1e-12 * means["saccades_sum"]
