"""Recurrence statistics on the device against the plain-loop restatement tests/recurrence_statistics_ref.py: the counts
and the RQA integers of scanpaths that exist exactly, the closed-form expectation bit for bit (NaN equal to NaN); the closed form
against the sampler's own kernel over all action sequences; the keyed functions, the table, the loop and the bootstrap."""
import itertools
from fractions import Fraction

import numpy as np
import pytest
import torch

import recurrence_statistics_ref as R

pytestmark = pytest.mark.gpu
MAPS = {(1, 1): (75.0, 100.0), (2, 2): (75.0, 100.0), (2, 3): (20.0, 45.0), (5, 7): (100.0, 300.0), (30, 40): (240.0, 320.0),
        (32, 64): (256.0, 512.0)}                                       # (5, 7) on 100 x 300: cells that are not square
_ROWS = {}


def M():
    from scanpaths_amd.utils.evaltools import recurrence_statistics
    return recurrence_statistics


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(-1)) if got.dtype.kind == "f" \
        else np.flatnonzero((got != want).reshape(-1))
    assert not len(bad), (what, len(bad), bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])


def radius_of(shape, kind):
    """0: the same cell only; "cell": the longer side of a cell, so the neighbours along both axes; "frame": every displacement"""
    fh, fw = MAPS[shape]
    return {"0": 0.0, "cell": max(fh / shape[0], fw / shape[1]), "frame": float(np.hypot(fh, fw))}[kind]


# ---- recurrence_counts --------------------------------------------------------------------------------------------------------------------
def count_paths(frame, seed=1):
    """lengths 0, 1, 2, 63, 64 off the pixel grid with fixations outside the frame; a cycle of four places walked 16 times (long
    diagonal lines), a dwell (horizontal and vertical lines), both again with a NaN and an out-of-frame fixation inside their lines;
    fixations on the frame's edges"""
    fh, fw = frame
    g = np.random.default_rng(seed)
    nan = float("nan")

    def path(n):
        return np.stack([g.uniform(-0.02 * fw, 1.02 * fw, n), g.uniform(-0.02 * fh, 1.02 * fh, n)], 1)

    paths = [path(n) for n in (0, 1, 2, 63, 64, 7, 9)]
    places = np.stack([g.uniform(0, fw, 4), g.uniform(0, fh, 4)], 1)
    cycle = np.tile(places, (16, 1)) + g.uniform(-0.4, 0.4, (64, 2))
    dwell = np.concatenate([np.tile(places[:1], (6, 1)), places[1:3], np.tile(places[:1], (5, 1)), places[3:], np.tile(places[1:2], (4, 1))])
    paths += [np.clip(cycle, 0, [np.nextafter(fw, 0), np.nextafter(fh, 0)]), dwell]
    for base in (cycle, dwell):
        p = np.clip(base, 0, [np.nextafter(fw, 0), np.nextafter(fh, 0)])
        p[3, 0], p[8, 1], p[len(p) - 1, 0] = nan, 2.0 * fh, -1.0
        paths.append(p)
    paths.append(np.array([(0.0, 0.0), (fw, 1.0), (1.0, 1.0), (1.0, fh), (np.nextafter(fw, 0), np.nextafter(fh, 0)), (0.0, fh / 2), (-0.0, 0.0),
                           (fw / 2, 0.0), (np.nextafter(0.0, -1), 1.0), (fw / 3, fh / 3)]))
    return paths


@pytest.mark.parametrize("min_line", [2, 3])
@pytest.mark.parametrize("max_steps", [1, 5, 64])
@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (5, 7), (30, 40)])
def test_counts_and_rqa_equal_the_restatement(shape, max_steps, min_line):
    frame = MAPS[shape]
    paths = count_paths(frame)
    groups = [k % 3 if k % 3 < 2 else 3 for k in range(len(paths))]     # group 2 of 4 stays empty
    radius = frame[1] / 6.0
    table = M().recurrence_mask(shape, frame, radius)
    got = M().recurrence_counts(paths, groups, 4, frame, shape, max_steps=max_steps, radius=radius, min_line=min_line)
    want = R.recurrence_counts(paths, groups, 4, frame, shape, max_steps, table, min_line)
    for k in ("counts", "points", "dropped", "rqa"):
        same(got[k], want[k], (k, shape, max_steps, min_line))
    assert set(got) == {"counts", "points", "dropped", "rqa"} and not got["counts"][2].any()
    upper, lower = np.triu(got["counts"], 1).sum(), np.tril(got["counts"], -1).sum()
    assert upper == want["points"].sum() and lower == (want["rqa"][:, 0] * (want["rqa"][:, 0] - 1) // 2).sum() >= upper
    assert np.trace(got["counts"], axis1=1, axis2=2).sum() == want["rqa"][:, 0].sum()
    assert got["points"][:2].tolist() == [0, 0] and (got["rqa"][:, 1] == got["points"]).all()
    if max_steps == 64:
        assert got["rqa"][7, 2] >= 100 and got["rqa"][8, 3] > 0 and got["rqa"][8, 4] > 0    # the cycle's diagonals, the dwell's lines
        assert got["dropped"][9:11].tolist() == [3, 3] and (got["rqa"][9, 1:3] < got["rqa"][7, 1:3]).all()   # fewer points, broken lines
    if shape == (1, 1):                                                  # one cell: every pair is recurrent
        assert np.array_equal(np.triu(got["counts"], 1), np.tril(got["counts"], -1).transpose(0, 2, 1))


@pytest.mark.parametrize("S", [1, 3, 4, 5])
def test_counts_blocks_with_idle_waves(S):
    frame, shape = MAPS[(5, 7)], (5, 7)
    paths = count_paths(frame, seed=2)[3:3 + S]
    table = M().recurrence_mask(shape, frame, 60.0)
    kw = dict(max_steps=64, radius=60.0, min_line=2)
    got = M().recurrence_counts(paths, [0] * S, 1, frame, shape, **kw)
    want = R.recurrence_counts(paths, [0] * S, 1, frame, shape, 64, table, 2)
    for k in got:
        same(got[k], want[k], (k, S))
    again = M().recurrence_counts(paths, [0] * S, 1, frame, shape, **kw)                    # the launcher zeroes the table every time
    same(again["counts"], want["counts"], "second call")


def test_counts_guard_themselves_at_the_c_entry_point():
    """a count the kernel cannot hold or a group that does not exist (the Python layer refuses both earlier): -1, nothing read or
    counted"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import _batch
    L = hip.stats_lib()
    rows = np.array([[1.0, 1.0], [12.0, 2.0], [3.0, 23.0], [3.0, 23.0]])
    counts = np.array([65, 3, -1, 4, 3, 3], dtype=np.int32)
    starts = np.array([0, 0, 0, 0, 1, 0], dtype=np.int64)               # (rows that would count, were they read)
    group = np.array([0, 1, 0, 0, 2, -1], dtype=np.int32)
    table = R.mask((3, 4), (30.0, 40.0), 0.0)
    buf, at = _batch.upload(dict(rows=rows, starts=starts, counts=counts, group=group, mask=table), dev())
    out = _batch.Out({"counts": (np.int64, 2 * 36), "points": (np.int32, 6), "dropped": (np.int32, 6), "rqa": (np.int32, 36)}, dev())
    hip.check(L.sp_stats_recurrence_counts(at["rows"], 2, at["starts"], at["counts"], at["group"], 6, 2, 6, 3, 4, 40.0, 30.0, at["mask"], 2,
                                           out.ptr("counts"), out.ptr("points"), out.ptr("dropped"), out.ptr("rqa"), hip.stream()),
              "sp_stats_recurrence_counts")
    host = out.host()
    assert host["points"].tolist() == [-1, 0, -1, 1, -1, -1] and host["dropped"].tolist() == [0] * 6
    assert host["rqa"].reshape(6, 6).tolist() == [[-1] * 6, [3, 0, 0, 0, 0, 0], [-1] * 6, [4, 1, 0, 0, 0, 1], [-1] * 6, [-1] * 6]
    want = R.recurrence_counts([rows[:3], rows[:4]], [1, 0], 2, (30.0, 40.0), (3, 4), 6, table, 2)["counts"]
    assert want[0, 2, 3] == 1 and want.sum() == 3 + 3 + 4 + 6 + 1
    same(host["counts"].reshape(2, 6, 6), want, "counts")


# ---- recurrence_expectation ---------------------------------------------------------------------------------------------------------------
def expect_case(shape, T):
    """raw positive float32 rows, not normalised, with p_0 <= Z at every step: 0 good, 1 a zero step at t = min(1, T - 1), 2 good, 3 a
    NaN cell at t = 0, 4 good"""
    key = (shape, T)
    if key not in _ROWS:
        P = shape[0] * shape[1]
        g = np.random.default_rng(100 * P + T)
        probs = g.uniform(0.01, 1.0, (5, T, 1 + P)).astype(np.float32)
        probs[:, :, 0] = (g.uniform(0.05, 0.9, (5, T)) * probs[:, :, 1:].min(2) * P).astype(np.float32)       # p_0 <= Z
        probs[1, min(1, T - 1), :] = 0.0
        probs[3, 0, 1 + P // 2] = float("nan")
        _ROWS[key] = (probs, {})
    return _ROWS[key]


def expect_reference(shape, T, kind, min_length, max_steps):
    """the restatement's per-row results, computed once per (case, radius, min_length, Tm) and shared"""
    probs, cache = expect_case(shape, T)
    key = (kind, min_length, min(T, max_steps))
    if key not in cache:
        table = M().recurrence_mask(shape, MAPS[shape], radius_of(shape, kind))
        cache[key] = R.recurrence_expectation(probs, [0] * len(probs), 1, table, min_length, max_steps)["rows"]
    return probs, cache[key]


# every map, every T and every radius once, not every triple; the large maps take few (min_length, max_steps): their restatement is
# what takes the time.  One cell; P below and above one pass of 256 threads and no multiple of 64; the 2048-cell limit; T = 1 (no pair)
EXPECT = [((1, 1), 1, "0"), ((1, 1), 3, "frame"), ((2, 3), 2, "cell"), ((2, 3), 16, "0"), ((5, 7), 3, "cell"), ((5, 7), 16, "frame"),
          ((30, 40), 2, "0"), ((30, 40), 16, "cell"), ((32, 64), 1, "cell"), ((32, 64), 3, "frame"), ((32, 64), 16, "0")]
BIG = {((30, 40), 2): ((0, 64), (3, 1)), ((30, 40), 16): ((2, 64), (0, 5)), ((32, 64), 1): ((0, 2),), ((32, 64), 3): ((1, 64), (0, 2)),
       ((32, 64), 16): ((2, 16),)}


@pytest.mark.parametrize("shape,T,kind", EXPECT)
def test_expectation_bit_for_bit(shape, T, kind):
    frame, radius = MAPS[shape], radius_of(shape, kind)
    table = M().recurrence_mask(shape, frame, radius)
    assert table.sum() == {"0": 1, "frame": table.size}.get(kind, table.sum()) and (kind != "cell" or table.size == 1 or table.sum() > 1)
    combos = BIG.get((shape, T)) or [(ml, ms) for ml in (0, 2, T + 1) for ms in (1, 2, 5, 64)]
    dp = torch.from_numpy(expect_case(shape, T)[0]).to(dev())
    for min_length, max_steps in combos:
        probs, rows = expect_reference(shape, T, kind, min_length, max_steps)
        for R_, groups, G in ((5, [0, 1, 0, 3, 0], 4), (1, [0], 1), (3, [1, 1, 0], 2)):
            # G = 4: group 2 is empty, group 3 holds only the NaN row, group 1 only the zero-step row
            got = M().recurrence_expectation(dp[:R_], groups, G, min_length=min_length, max_steps=max_steps, radius=radius, frame_size=frame,
                                             map_shape=shape)
            want = R.recurrence_expectation(probs[:R_], groups, G, table, min_length, max_steps, rows=rows[:R_])
            for k in ("E", "points", "bad"):
                same(got[k], want[k], (k, shape, T, kind, min_length, max_steps, R_))
            Tm = min(T, max_steps)
            bad = [0, int(Tm > min(1, T - 1)), 0, 1, 0][:R_]
            assert got["bad"].tolist() == bad and np.isnan(got["points"]).tolist() == [b == 1 for b in bad]
            assert got["E"].shape == (G, max_steps, max_steps) and not got["E"][:, Tm:].any() and not got["E"][:, :, Tm:].any()
            assert got["E"][0 if G != 2 else 1, 0, 0] > 0
            if Tm < 2:
                assert (got["points"][np.array(bad) == 0] == 0).all()
            if G == 4:
                assert not got["E"][2].any() and not got["E"][3].any()
            if kind == "frame":                                          # every pair that exists is recurrent, up to the rounding of X
                up, low = np.triu(got["E"][0], 1), np.tril(got["E"][0], -1).T
                assert np.allclose(up, low, rtol=(2 * shape[0] * shape[1] + 8) * 2.0 ** -53, atol=0)


def test_expectation_guards_itself_at_the_c_entry_point():
    """a row_group outside [0, ngroups) (the Python layer refuses it earlier): bad -1, NaN, nothing of the row is read or added; a mask
    entry other than 0 and 1 counts as 1"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import _batch
    shape, T = (5, 7), 3
    probs, _ = expect_case(shape, T)
    L = hip.stats_lib()
    groups = np.array([0, 5, -1, 1, 0], dtype=np.int32)
    table = M().recurrence_mask(shape, MAPS[shape], radius_of(shape, "cell"))
    table[table > 0] = np.arange(1, table.sum() + 1, dtype=np.uint8) * 50 % 255 + 1
    D = table.size
    buf, at = _batch.upload({"row_group": groups, "mask": table}, dev())
    dp = torch.from_numpy(probs).to(dev())
    work = torch.empty(5 * 9 + D // 2 + 1, dtype=torch.float64, device=dev())
    out = _batch.Out({"E": (np.float64, 2 * 16), "points": (np.float64, 5), "bad": (np.int32, 5)}, dev())
    hip.check(L.sp_stats_recurrence_expectation(hip.ptr(dp), at["row_group"], 5, T, 5, 7, 2, 1, 4, at["mask"], hip.ptr(work), out.ptr("E"),
                                                out.ptr("points"), out.ptr("bad"), hip.stream()), "sp_stats_recurrence_expectation")
    host = out.host()
    want = R.recurrence_expectation(probs, groups, 2, (table > 0).astype(np.uint8), 1, 4)
    assert want["bad"].tolist() == [0, -1, -1, 1, 0]
    for k in ("points", "bad"):
        same(host[k], want[k], k)
    same(host["E"].reshape(2, 4, 4), want["E"], "E")


def test_expectation_keeps_probs_on_the_device_and_reads_any_float_dtype():
    shape, T, kind = (5, 7), 3, "cell"
    frame, radius = MAPS[shape], radius_of(shape, kind)
    probs, rows = expect_reference(shape, T, kind, 0, 64)
    dp = torch.from_numpy(probs[[0, 2]]).to(dev())
    want = R.recurrence_expectation(probs[[0, 2]], [0, 0], 1, M().recurrence_mask(shape, frame, radius), 0, 64, rows=[rows[0], rows[2]])
    kw = dict(min_length=0, max_steps=64, radius=radius, frame_size=frame)
    for tensor in (dp, dp.double(), dp.expand(2, T, 36).transpose(0, 1).contiguous().transpose(0, 1)):
        same(M().recurrence_expectation(tensor, [0, 0], 1, map_shape=shape, **kw)["E"], want["E"], str(tensor.dtype))
    with pytest.raises(ValueError, match="map_shape is required"):
        M().recurrence_expectation(dp, [0, 0], 1, **kw)
    p1201 = torch.rand(1, 3, 1201, device=dev())
    assert M().recurrence_expectation(p1201, [0], 1, **dict(kw, frame_size=(240, 320), radius=16.0, max_steps=3))["E"].shape == (1, 3, 3)


# ---- the closed form against the sampler's own kernel ------------------------------------------------------------------------------------
def test_sampled_and_exact_forms_agree_over_all_sequences():
    """all 5^3 action sequences of a T = 3, 2 x 2 case on 75 x 100 go through Sampling.generate_scanpath and recurrence_counts (one
    group per sequence); weighted by their exact probabilities they give the closed form within the enumeration's bound
    ((1 + P)^T + T) * 2^-53 relative, entry by entry -- recurrent pairs, pairs and fixations"""
    from scanpaths_amd.models.sampling import Sampling
    T, Hm, Wm, min_length = 3, 2, 2, 1
    frame, radius = (75.0, 100.0), 40.0                                  # cells of 50 x 37.5: the cell and its vertical neighbour
    g = np.random.default_rng(31)
    probs = g.uniform(0.05, 1.0, (2, T, 5)).astype(np.float32)
    seqs = np.array(list(itertools.product(range(5), repeat=T)), dtype=np.int64)
    s = Sampling(convLSTM_length=T, min_length=min_length, map_width=Wm, map_height=Hm, width=100, height=75)
    fvs, _, _ = s.generate_scanpath(torch.zeros(1), None, torch.ones(len(seqs), T, device=dev()), torch.from_numpy(seqs).to(dev()))
    paths = [np.stack([fv["start_x"], fv["start_y"]], 1) for fv in fvs]
    counts = M().recurrence_counts(paths, np.arange(len(seqs)), len(seqs), frame, (Hm, Wm), max_steps=T, radius=radius, min_line=2)
    assert (counts["dropped"] == 0).all() and counts["counts"].shape == (125, T, T)
    assert M().recurrence_mask((Hm, Wm), frame, radius).tolist() == [[0, 1, 0], [0, 1, 0], [0, 1, 0]]
    exact = M().recurrence_expectation(torch.from_numpy(probs).to(dev()), [0, 1], 2, min_length=min_length, max_steps=T, radius=radius,
                                       frame_size=frame, map_shape=(Hm, Wm))
    bound = (5 ** T + T) * 2.0 ** -53
    for row in range(2):
        table = [[Fraction(0)] * T for _ in range(T)]
        total = Fraction(0)
        for k, seq in enumerate(seqs):
            w = Fraction(1)
            for t, a in enumerate(seq):
                allowed = range(1, 5) if t < min_length else range(5)
                w *= Fraction(float(probs[row, t, a])) / sum(Fraction(float(probs[row, t, j])) for j in allowed) if a in allowed else 0
            total += w
            n = len(list(itertools.takewhile(lambda a: a != 0, seq)))
            if w:
                assert np.array_equal(np.tril(counts["counts"][k]), np.tril(np.ones((T, T), np.int64)) * (np.arange(T)[:, None] < n)), seq
            for r in range(T):
                for c in range(T):
                    if counts["counts"][k, r, c]:
                        table[r][c] += w * int(counts["counts"][k, r, c])
        assert total == 1
        for r in range(T):
            for c in range(T):
                want = float(table[r][c])
                assert abs(want - exact["E"][row, r, c]) <= bound * want, (row, r, c, want, exact["E"][row, r, c])
        points = float(sum(table[r][c] for r in range(T) for c in range(r + 1, T)))
        assert points > 0 and abs(points - exact["points"][row]) <= bound * points


# ---- keyed calls, the table, the loop, the bootstrap -------------------------------------------------------------------------------------
EV = dict(frame_size=(240, 320), map_shape=(30, 40), max_steps=8, radius=60.0, min_line=2)


def _keyed_case():
    g = np.random.default_rng(41)
    keys = ["q1", "q2", "q3", "q4"]

    def path():
        n = int(g.integers(0, 11))
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


def test_keyed_evaluation_human_row_groups_table_merge_and_bootstrap():
    from scanpaths_amd.utils import evaluation as E
    keys, gt, gt_keys, pred, pred_keys = _keyed_case()
    tasks = {"q1": "cup", "q2": "fork", "q3": "cup", "q4": "fork"}
    table = M().recurrence_mask(EV["map_shape"], EV["frame_size"], EV["radius"])
    means, per_key = E.recurrence_statistics_evaluation(gt, pred, gt_keys, pred_keys, groups=tasks, **EV)
    assert per_key["keys"] == keys and set(means["by_group"]) == {"cup", "fork"}
    for prefix, paths, pk in (("", pred, pred_keys), ("human_", gt, gt_keys)):
        res = R.recurrence_counts([p[:, :2] for p in paths], [0] * len(paths), 1, EV["frame_size"], EV["map_shape"], 8, table, 2)
        same(means[prefix + "table_sum"], res["counts"][0], prefix + "table")
        assert means[prefix + "points_sum"] == res["points"].sum() == np.triu(means[prefix + "table_sum"], 1).sum() > 0
        assert means[prefix + "fixations_dropped"] == res["dropped"].sum() > 0 and means[prefix + "scanpaths_count"] == len(paths)
        _equal(means[prefix + "summary"], M().recurrence_summary(res["counts"][0]), prefix + "summary")
        scores = [R.measures(row) for row in res["rqa"]]
        for q, k in enumerate(keys):
            mine = np.array([kk == k for kk in pk])
            assert per_key[prefix + "points"][q] == res["points"][mine].sum() and per_key[prefix + "dropped"][q] == res["dropped"][mine].sum()
            for name in ("REC", "DET", "LAM", "CORM"):
                values = [s[name] for s, m in zip(scores, mine) if m and not np.isnan(s[name])]
                want = sum(values) / len(values) if values else float("nan")
                got = per_key[prefix + name][q]
                assert (np.isnan(got) and np.isnan(want)) or abs(got - want) <= 1e-12 * abs(want), (prefix, name, k, got, want)
        assert per_key[prefix + "REC"].dtype == np.float64 and not np.isnan(per_key[prefix + "REC"]).all()
        for task in ("cup", "fork"):
            mine = [i for i, k in enumerate(pk) if tasks[k] == task]
            part = R.recurrence_counts([paths[i][:, :2] for i in mine], [0] * len(mine), 1, EV["frame_size"], EV["map_shape"], 8, table, 2)
            same(means["by_group"][task][prefix + "table_sum"], part["counts"][0], (prefix, task))
        same(sum(means["by_group"][task][prefix + "table_sum"] for task in ("cup", "fork")), means[prefix + "table_sum"], "groups sum")
    want = M().recurrence_comparison(means["table_sum"], means["human_table_sum"])
    assert set(want) == {"REC_difference", "L1_by_lag", "JSD_lag"} and all(means[k] == v for k, v in want.items())
    assert 0 <= means["JSD_lag"] <= 1 and set(want) <= set(means["by_group"]["cup"])
    assert not any(isinstance(v, np.ndarray) and v.ndim > 1 for v in per_key.values())      # no table per key
    # the human-only call equals the human half of the full call
    human, human_keys = E.recurrence_statistics_human_evaluation(gt, gt_keys, groups=tasks, **EV)
    assert set(human) == {k for k in means if k.startswith("human_")} | {"by_group"}
    for k, v in human.items():
        if k != "by_group":
            _equal(v, means[k], k)
    for task, part in human["by_group"].items():
        _equal(part, {k: v for k, v in means["by_group"][task].items() if k.startswith("human_")}, task)
    assert np.array_equal(human_keys["human_points"], per_key["human_points"])
    assert np.array_equal(human_keys["human_REC"], per_key["human_REC"], equal_nan=True)
    # two batches merged by the table equal one call on their union, exactly: every merged entry is an integer
    merged = E.RecurrenceStatisticsTable(EV["max_steps"])
    for part in (("q1", "q2"), ("q3", "q4")):
        gi, pi = [i for i, k in enumerate(gt_keys) if k in part], [i for i, k in enumerate(pred_keys) if k in part]
        merged.add(E.recurrence_statistics_evaluation([gt[i] for i in gi], [pred[i] for i in pi], [gt_keys[i] for i in gi],
                                                      [pred_keys[i] for i in pi], groups=tasks, **EV)[0])
    _equal(merged.result(), means, "table")
    pooled, _ = E.recurrence_statistics_evaluation(gt, pred, gt_keys, pred_keys, **EV)      # the default: one pooled group
    _equal(pooled, {k: v for k, v in means.items() if k != "by_group"}, "pooled")
    # the bootstrap runs on the new per_key columns as on every other family's
    names = ["human_REC", "human_DET", "human_LAM", "human_CORM", "REC", "DET", "LAM", "CORM"]
    res = E.bootstrap_evaluation(per_key, replicates=100, seed=5)
    assert list(res) == names
    for name in names:
        column = per_key[name]
        if not np.isnan(column).all():
            assert abs(res[name]["estimate"] - np.nanmean(column)) <= 1e-12 * abs(np.nanmean(column)) and res[name]["n_valid"] > 0
            assert res[name]["lo"] <= res[name]["hi"]
    paired = E.bootstrap_comparison(per_key, per_key, names=["REC"], replicates=50, seed=5)
    assert paired["REC"]["difference"] == 0.0


def test_model_evaluation_heads_groups_and_table(monkeypatch):
    from scanpaths_amd.utils import evaluation as E
    g = np.random.default_rng(51)
    N, T, shape, frame, radius = 4, 5, (6, 8), (48, 64), 8.0
    A = 1 + shape[0] * shape[1]
    mk = lambda: g.dirichlet(np.ones(A), (N, T)).astype(np.float32)                         # noqa: E731
    host = {"all_actions_prob": mk(), "good_all_actions_prob": mk(), "poor_all_actions_prob": mk()}
    host["all_actions_prob"][3, 1, 1:] = 0.0                                                # sample 3: a step without cell mass,
    predict = {k: torch.from_numpy(v).to(dev()) for k, v in host.items()}
    keys = ["a", "b", "a", "c"]
    performances = [[True, False, True], [False], [], [True, True]]
    kw = dict(min_length=2, max_steps=4, radius=radius, frame_size=frame, map_shape=shape)  # bad, as terminate is masked at t = 1
    table = M().recurrence_mask(shape, frame, radius)
    # one head
    means, per_key = E.recurrence_statistics_model_evaluation(predict, keys, **kw)
    want = R.recurrence_expectation(host["all_actions_prob"], [0] * N, 1, table, 2, 4)
    same(means["table_sum"], want["E"][0], "table_sum")
    assert want["bad"].tolist() == [0, 0, 0, 1] and means["rows_count"] == 3 and means["rows_bad"] == 1 and per_key["keys"] == ["a", "b", "c"]
    assert means["points_sum"] == float(want["points"][:3].sum()) and set(means) == {"table_sum", "points_sum", "rows_count", "rows_bad", "summary"}
    same(per_key["points"], np.array([(want["points"][0] + want["points"][2]) / 2, want["points"][1], np.nan]), "per key")
    _equal(means["summary"], M().recurrence_summary(means["table_sum"]), "summary")
    human = g.integers(1, 9, (4, 4))
    full = E.recurrence_statistics_model_evaluation(predict, keys, human_table=human, groups={"a": 0, "b": 1, "c": 0}, **kw)[0]
    assert all(full[k] == v for k, v in M().recurrence_comparison(full["table_sum"], human).items())
    by = R.recurrence_expectation(host["all_actions_prob"], [0, 1, 0, 0], 2, table, 2, 4, rows=want["rows"])
    same(full["by_group"][0]["table_sum"], by["E"][0], "label 0")
    same(full["by_group"][1]["table_sum"], by["E"][1], "label 1")
    assert full["by_group"][0]["rows_bad"] == 1 and full["by_group"][1]["rows_count"] == 1 and "JSD_lag" not in full["by_group"][0]
    same(full["by_group"][0]["table_sum"] + full["by_group"][1]["table_sum"], full["table_sum"], "the groups' tables sum to the pooled one")
    assert np.allclose(full["table_sum"], means["table_sum"], rtol=4 * 2.0 ** -53, atol=0)              # (E_0 + E_2) + E_1 against row order
    # the two AiR heads: the rows are the ones turn_statistics_model_evaluation reads for the same performances
    seen = {}
    real = M().recurrence_expectation

    def spy(probs, row_groups, n_groups, **k):
        seen["probs"] = probs.cpu().numpy()
        return real(probs, row_groups, n_groups, **k)

    monkeypatch.setattr(M(), "recurrence_expectation", spy)
    means2, per_key2 = E.recurrence_statistics_model_evaluation(predict, keys, performances=performances, **kw)
    both = np.concatenate([host["good_all_actions_prob"], host["poor_all_actions_prob"]], 0)
    rows = [0, N + 0, 0, N + 1, 3, 3]                                                       # built by hand from performances
    assert np.array_equal(seen["probs"], both[rows])
    want2 = R.recurrence_expectation(both[rows], [0] * 6, 1, table, 2, 4)
    same(means2["table_sum"], want2["E"][0], "two heads")
    assert means2["rows_count"] == 6 and means2["rows_bad"] == 0 and np.isnan(per_key2["points"]).tolist() == [False, False, False]
    # the table over two batches equals one call on their union within 4 * 2^-53 relative per added table (two here): both are sums
    # of the same N <= 4 non-negative E_r per entry in two associations, each within N * 2^-53 relative of the true sum
    merged = E.RecurrenceStatisticsTable(4)
    for lo in (0, 2):
        sl = {k: v[lo:lo + 2] for k, v in predict.items()}
        merged.add(E.recurrence_statistics_model_evaluation(sl, keys[lo:lo + 2], **kw)[0])
    out = merged.result(human)
    assert out["rows_count"] == 3 and out["rows_bad"] == 1
    assert np.allclose(out["table_sum"], means["table_sum"], rtol=2 * 4 * 2.0 ** -53, atol=0)
    assert abs(out["points_sum"] - means["points_sum"]) <= 2 * 4 * 2.0 ** -53 * means["points_sum"]
    assert out["JSD_lag"] == M().recurrence_comparison(out["table_sum"], human)["JSD_lag"] and abs(out["JSD_lag"] - full["JSD_lag"]) <= 1e-12
    res = E.bootstrap_evaluation(per_key2, replicates=50, seed=3)
    assert list(res) == ["points"] and res["points"]["n_valid"] == 50


def test_recurrence_statistics_loop_on_a_tiny_multihead_model(monkeypatch):
    from scanpaths_amd import hip, inference
    from scanpaths_amd.models.baseline_attention_multihead import baseline
    from scanpaths_amd.procedural import fill_module
    from scanpaths_amd.synth import make_batch
    from scanpaths_amd.utils import evaluation as E
    T, B, radius = 3, 2, 16.0
    batches = [make_batch("COCO_Search18", B, 240, 320, T, seed=9 + k) for k in range(2)]
    model = baseline(convLSTM_length=T)
    fill_module(model, 9, family="tame")
    model = model.to(dev())
    loader = [{"images": b["images"], "attention_maps": b["attention_maps"], "tasks": b["tasks"], "question_ids": [f"s{2 * k}", f"s{2 * k + 1}"]}
              for k, b in enumerate(batches)]
    L, S = hip.lib(), hip.stats_lib()
    launches, launch = [], S.sp_stats_recurrence_expectation
    monkeypatch.setattr(S, "sp_stats_recurrence_expectation", lambda *a: launches.append(1) or launch(*a))
    for name in ("sp_sample_actions", "sp_generate_scanpath", "sp_beam_search"):
        monkeypatch.setattr(L, name, lambda *a: (_ for _ in ()).throw(AssertionError("the recurrence-statistics loop does not sample")))
    human = np.random.default_rng(2).integers(1, 5, (3, 3))
    means, per_batch = inference.run_recurrence_statistics_loop(model, loader, min_length=1, max_steps=3, radius=radius, human_table=human)
    assert len(launches) == 2 and len(per_batch) == 2 and per_batch[1]["keys"] == ["s2", "s3"] and not model.training
    table = E.RecurrenceStatisticsTable(3)
    for k, b in enumerate(batches):
        with torch.no_grad():
            predict = model(b["images"].to(dev()), b["attention_maps"].to(dev()), b["tasks"].to(dev()))
        assert tuple(predict["all_actions_prob"].shape) == (B, T, 1201)
        direct = M().recurrence_expectation(predict["all_actions_prob"], [0, 0], 1, min_length=1, max_steps=3, radius=radius, frame_size=(240, 320))
        ev, keyed = E.recurrence_statistics_model_evaluation(predict, loader[k]["question_ids"], min_length=1, max_steps=3, radius=radius)
        same(ev["table_sum"], direct["E"][0], "evaluation")
        same(keyed["points"], direct["points"], "per key")
        same(per_batch[k]["points"], direct["points"], "loop per key")
        table.add(ev)
    _equal(means, table.result(human), "the loop returns the table of its batches")
    assert means["rows_count"] == 4 and 0 < means["points_sum"] <= 4 * 3 and 0 <= means["JSD_lag"] <= 1
    assert abs(means["summary"]["points"] - means["points_sum"]) <= 1e-12 * means["points_sum"]
    assert means["summary"]["fixations"] <= 4 * 3 and 0 <= means["summary"]["REC"] <= 100
