"""CPU-only checks of the saccade-statistics layer: the two entry points are declared, bound and exported with equal
signatures and refuse bad arguments before any launch; every argument refusal of the Python layer is raised before a device or the
library is touched; the Python restatement of the closed form (tests/saccade_statistics_ref.py) equals the exhaustive enumeration of
all action sequences under the sampler's rule in exact rational arithmetic -- which makes it independent of the closed form's own
reasoning -- and the host statistics hold answers worked out by hand."""
import inspect
import itertools
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import abi
import saccade_statistics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sp_scan_saccade_counts": ("int", 16), "sp_scan_saccade_expectation": ("int", 14)}


def M():
    from scanpaths_amd.utils.evaltools import saccade_statistics
    return saccade_statistics


def test_new_entry_points_are_declared_bound_and_exported():
    lib = abi.assert_declared(NEW, prefixes=("sp_scan_saccade_",))
    assert lib.sp_scan_max_fixations() == M().MAX_FIXATIONS == R.MAX_FIXATIONS == 64
    assert lib.sp_scan_likelihood_max_cells() == M().MAX_CELLS == R.MAX_CELLS == 2048
    assert "scansaccade.hip" in open(os.path.join(ROOT, "scanpaths_amd", "csrc", "Makefile")).read()


def test_launchers_refuse_bad_arguments_without_a_device():
    """SP_ENULL (-2) / SP_EINVAL (-1) come before the launch, so on a machine without a GPU too.  Every call below is a refused one."""
    lib = abi.raw_lib()
    p = 4096                                                        # any non-NULL value: nothing is dereferenced before the checks
    nan, inf = float("nan"), float("inf")

    def with_(call, base, **kw):
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)

    # sp_scan_saccade_counts(fix, ncol, start, count, group, nscan, ngroups, max_steps, Hm, Wm, frame_w, frame_h, counts, saccades, dropped, stream)
    ok = [p, 2, p, p, p, 5, 2, 6, 30, 40, 320.0, 240.0, p, p, p, None]
    counts = lib.sp_scan_saccade_counts
    for k in (0, 2, 3, 4, 12, 13, 14):                              # inputs and every output
        assert with_(counts, ok, **{f"a{k}": None}) == -2, k
    for k, bad in ((1, 1), (1, 0), (1, -2), (5, 0), (5, -1), (6, 0), (6, -1), (7, 0), (7, -3), (8, 0), (8, -30), (9, 0), (9, -1),
                   (8, 52), (9, 69), (8, 1 << 20), (10, 0.0), (10, -1.0), (10, nan), (10, inf), (11, 0.0), (11, -2.0), (11, nan), (11, inf)):
        assert with_(counts, ok, **{f"a{k}": bad}) == -1, (k, bad)  # 52 x 40 = 2080 and 30 x 69 = 2070 cells: above 2048
    assert with_(counts, ok, a0=None, a1=1) == -2                   # NULL is answered before a bad scalar
    # sp_scan_saccade_expectation(probs, row_group, R, T, Hm, Wm, ngroups, min_length, max_steps, work, E, saccades, bad, stream)
    ok = [p, p, 3, 4, 30, 40, 2, 1, 6, p, p, p, p, None]
    exp = lib.sp_scan_saccade_expectation
    for k in (0, 1, 9, 10, 11, 12):
        assert with_(exp, ok, **{f"a{k}": None}) == -2, k
    for k, bad in ((2, 0), (2, -1), (3, 0), (3, -2), (4, 0), (4, -30), (4, 52), (5, 0), (5, 69), (5, 1 << 20), (6, 0), (6, -1), (7, -1),
                   (8, 0), (8, -5)):
        assert with_(exp, ok, **{f"a{k}": bad}) == -1, (k, bad)
    assert with_(exp, ok, a1=None, a2=0) == -2                      # NULL is answered before a bad scalar
    assert with_(exp, ok, a4=32, a5=65) == -1                       # 2080 cells


def test_public_surface():
    from scanpaths_amd import inference
    from scanpaths_amd.utils import evaluation as E
    empty, KW = inspect.Parameter.empty, inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(M().saccade_counts).parameters
    assert list(p) == ["scanpaths", "groups", "n_groups", "frame_size", "map_shape", "max_steps"]
    assert p["max_steps"].kind is KW and all(p[k].default is empty for k in p)
    p = inspect.signature(M().saccade_expectation).parameters
    assert list(p) == ["probs", "row_groups", "n_groups", "min_length", "max_steps", "map_shape"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("min_length", "max_steps")) and p["map_shape"].default is None
    p = inspect.signature(M().saccade_summary).parameters
    assert list(p) == ["lattice", "frame_size", "amplitude_edges", "n_directions"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("amplitude_edges", "n_directions"))
    p = inspect.signature(E.saccade_statistics_evaluation).parameters
    assert list(p) == ["gt_fix_vectors", "predict_fix_vectors", "gt_keys", "predict_keys", "frame_size", "map_shape", "max_steps",
                       "amplitude_edges", "n_directions", "groups", "image_keys"]
    assert all(p[k].kind is KW and p[k].default is empty for k in list(p)[4:9]) and p["groups"].default is None
    p = inspect.signature(E.saccade_statistics_model_evaluation).parameters
    assert list(p)[:9] == ["predict", "keys", "min_length", "max_steps", "performances", "frame_size", "map_shape", "groups", "human_lattice"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("min_length", "max_steps")) and p["frame_size"].default == (240, 320)
    assert list(inspect.signature(E.SaccadeStatisticsTable.__init__).parameters) == ["self", "frame_size", "map_shape", "amplitude_edges",
                                                                                      "n_directions"]
    assert list(inspect.signature(E.SaccadeStatisticsTable.result).parameters) == ["self", "human_lattice"]
    p = inspect.signature(inference.run_saccade_statistics_loop).parameters
    assert list(p) == ["model", "loader", "min_length", "max_steps", "amplitude_edges", "n_directions", "human_lattice",
                       "ablate_attention_info", "frame_size", "map_shape"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("min_length", "max_steps", "amplitude_edges", "n_directions"))
    assert list(inspect.signature(E.SearchEfficiencyTable.result).parameters) == ["self", "human_curve"]       # the older table stays


def test_refusals_come_before_any_device_call(monkeypatch):
    from scanpaths_amd import hip, inference
    from scanpaths_amd.utils import evaluation as E

    def no_lib():
        raise AssertionError("validation must come first")

    monkeypatch.setattr(M(), "_device", no_lib)
    monkeypatch.setattr(hip, "lib", no_lib)
    sp = np.array([[1.0, 1.0, 0.2], [5.0, 3.0, 0.3]])
    frame, shape = (24, 40), (3, 5)
    counts = M().saccade_counts
    with pytest.raises(TypeError):
        counts([sp], [0], 1, frame, shape)                                                  # max_steps has no default
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="max_steps"):
            counts([sp], [0], 1, frame, shape, max_steps=bad)
    with pytest.raises(ValueError, match="kernel limit"):
        counts([np.zeros((M().MAX_FIXATIONS + 1, 2))], [0], 1, frame, shape, max_steps=6)   # a scanpath of 65
    for bad in ((0, 5), (3,), (3, -5), (2.5, 4), None, (3, 5, 7)):
        with pytest.raises(ValueError, match="map_shape"):
            counts([sp], [0], 1, frame, bad, max_steps=6)
    with pytest.raises(ValueError, match="kernel limit"):
        counts([sp], [0], 1, frame, (32, 65), max_steps=6)                                  # 2080 cells
    for bad in ([1], [-1], [2]):
        with pytest.raises(ValueError, match="out of range"):
            counts([sp], bad, 1, frame, shape, max_steps=6)
    with pytest.raises(ValueError, match="one group per scanpath"):
        counts([sp, sp], [0], 1, frame, shape, max_steps=6)
    for bad in (0, -1, None, 1.5):
        with pytest.raises(ValueError, match="n_groups"):
            counts([sp], [0], bad, frame, shape, max_steps=6)
    for bad in ((0, 32), (24, float("inf")), (float("nan"), 32)):
        with pytest.raises(ValueError, match="frame_size"):
            counts([sp], [0], 1, bad, shape, max_steps=6)
    with pytest.raises(ValueError, match="scanpath is an"):
        counts([np.zeros((3, 1))], [0], 1, frame, shape, max_steps=6)
    res = counts([], [], 2, frame, shape, max_steps=3)                                      # nothing to count: zeros, no device
    assert res["counts"].dtype == np.int64 and res["counts"].shape == (2, 5, 9) and not res["counts"].any()
    assert res["saccades"].dtype == res["dropped"].dtype == np.int32 and res["saccades"].shape == (0,)

    T = 4
    probs = torch.full((2, T, 16), 1.0 / 16)
    exp = M().saccade_expectation
    with pytest.raises(TypeError):
        exp(probs, [0, 0], 1, max_steps=4, map_shape=shape)                                 # min_length has no default
    with pytest.raises(TypeError):
        exp(probs, [0, 0], 1, min_length=1, map_shape=shape)                                # nor has max_steps
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="min_length"):
            exp(probs, [0, 0], 1, min_length=bad, max_steps=4, map_shape=shape)
    for bad in (0, 2.5, None):
        with pytest.raises(ValueError, match="max_steps"):
            exp(probs, [0, 0], 1, min_length=1, max_steps=bad, map_shape=shape)
    with pytest.raises(ValueError, match="probs"):
        exp(probs[0], [0, 0], 1, min_length=1, max_steps=4, map_shape=shape)
    with pytest.raises(ValueError, match="probs"):
        exp(probs.numpy(), [0, 0], 1, min_length=1, max_steps=4, map_shape=shape)
    with pytest.raises(ValueError, match="map_shape is required"):
        exp(probs, [0, 0], 1, min_length=1, max_steps=4)
    for bad in ((4, 4), (3, 6), (0, 15), (-3, -5)):
        with pytest.raises(ValueError, match="map_shape"):
            exp(probs, [0, 0], 1, min_length=1, max_steps=4, map_shape=bad)
    with pytest.raises(ValueError, match="kernel limit"):
        exp(torch.zeros(1, 2, 2081), [0], 1, min_length=1, max_steps=4, map_shape=(32, 65))
    for bad in ([0, 1], [-1, 0]):
        with pytest.raises(ValueError, match="out of range"):
            exp(probs, bad, 1, min_length=1, max_steps=4, map_shape=shape)
    with pytest.raises(ValueError, match="one group per row"):
        exp(probs, [0], 1, min_length=1, max_steps=4, map_shape=shape)

    lattice = np.zeros((5, 9))
    for fn in (lambda **kw: M().saccade_summary(lattice, frame, **kw),):
        with pytest.raises(TypeError):
            fn(n_directions=4)
        with pytest.raises(TypeError):
            fn(amplitude_edges=[0.0, 1.0])
        for bad in (None, [1.0], [0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, float("nan")]):
            with pytest.raises(ValueError, match="amplitude_edges"):
                fn(amplitude_edges=bad, n_directions=4)
        for bad in (0, -1, 2.5, None, True):
            with pytest.raises(ValueError, match="n_directions"):
                fn(amplitude_edges=[0.0, 1.0], n_directions=bad)
    with pytest.raises(ValueError, match="lattice"):
        M().saccade_summary(np.zeros((4, 9)), frame, amplitude_edges=[0.0, 1.0], n_directions=4)

    # the keyed layer
    ev = E.saccade_statistics_evaluation
    kw = dict(frame_size=frame, map_shape=shape, max_steps=3, amplitude_edges=[0.0, 8.0, 16.0], n_directions=4)
    for missing in ("frame_size", "map_shape", "max_steps", "amplitude_edges", "n_directions"):
        with pytest.raises(TypeError):
            ev([sp], [sp], ["a"], ["a"], **{k: v for k, v in kw.items() if k != missing})
    with pytest.raises(ValueError, match="amplitude_edges"):
        ev([sp], [sp], ["a"], ["a"], **dict(kw, amplitude_edges=[3.0, 2.0]))
    with pytest.raises(ValueError, match="n_directions"):
        ev([sp], [sp], ["a"], ["a"], **dict(kw, n_directions=0))
    with pytest.raises(ValueError, match="one key per fixation vector"):
        ev([sp, sp], [sp], ["a"], ["a"], **kw)
    with pytest.raises(ValueError, match="not among gt_keys"):
        ev([sp], [sp], ["a"], ["b"], **kw)
    with pytest.raises(ValueError, match="'b'.*has no group"):
        ev([sp, sp], [sp], ["a", "b"], ["a"], groups={"a": "t"}, **kw)
    with pytest.raises(ValueError, match="two images"):
        ev([sp, sp], [sp], ["a", "a"], ["a"], image_keys=["i", "j"], **kw)
    with pytest.raises(ValueError, match="kernel limit"):
        ev([np.zeros((65, 2))], None, ["a"], None, **kw)
    one = {"all_actions_prob": probs}
    two = {"good_all_actions_prob": probs, "poor_all_actions_prob": probs}
    mv = E.saccade_statistics_model_evaluation
    mkw = dict(min_length=1, max_steps=3, frame_size=frame, map_shape=shape)
    with pytest.raises(TypeError):
        mv(one, ["a", "b"], max_steps=3)
    with pytest.raises(TypeError):
        mv(one, ["a", "b"], min_length=1)
    with pytest.raises(ValueError, match="predict lacks 'good_all_actions_prob'"):
        mv(one, ["a", "b"], performances=[[True], [False]], **mkw)
    with pytest.raises(ValueError, match="predict lacks 'all_actions_prob'"):
        mv(two, ["a", "b"], **mkw)
    with pytest.raises(ValueError, match="one list of performances per sample"):
        mv(two, ["a", "b"], performances=[[True]], **mkw)
    with pytest.raises(ValueError, match="samples"):
        mv(one, ["a", "b", "a"], **mkw)
    with pytest.raises(ValueError, match="map_shape"):
        mv(one, ["a", "b"], min_length=1, max_steps=3)
    with pytest.raises(ValueError, match="go together"):
        mv(one, ["a", "b"], amplitude_edges=[0.0, 1.0], **mkw)
    with pytest.raises(ValueError, match="human_lattice"):
        mv(one, ["a", "b"], human_lattice=np.ones((5, 9)), **mkw)
    with pytest.raises(ValueError, match="has no group"):
        mv(one, ["a", "b"], groups={"a": 0}, **mkw)
    with pytest.raises(ValueError, match="amplitude_edges"):
        E.SaccadeStatisticsTable(frame, shape, [1.0], 4)
    with pytest.raises(ValueError, match="amplitude_edges"):
        inference.run_saccade_statistics_loop(None, [], min_length=1, max_steps=3, amplitude_edges=[2.0, 1.0], n_directions=4)
    with pytest.raises(ValueError, match="n_directions"):
        inference.run_saccade_statistics_loop(None, [], min_length=1, max_steps=3, amplitude_edges=[0.0, 1.0], n_directions=0)


def test_no_cpu_path(monkeypatch):
    from scanpaths_amd import hip
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(hip.HipError, match="no CPU path"):
        M().saccade_counts([np.array([[1.0, 1.0]])], [0], 1, (24, 32), (3, 4), max_steps=2)
    with pytest.raises(hip.HipError, match="no CPU path"):
        M().saccade_expectation(torch.zeros(1, 2, 13), [0], 1, min_length=0, max_steps=2, map_shape=(3, 4))


# ---- the restatement against exhaustive enumeration ------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,shape", [(3, (2, 2)), (4, (2, 3))])
def test_restatement_equals_the_exhaustive_enumeration(T, shape):
    """All (1 + P)^T action sequences under the sampler's rule (terminate masked for t < min_length, the first terminate ends the
    scanpath), weighted in exact rationals: the expected number of saccades per displacement, entry by entry, to 1e-15 absolute; the
    restatement's "saccades" equals its lattice total.  (Every entry is a sum of at most (T - 1) P products of probabilities that sum
    to at most T - 1; a double sum of so few terms below 3 carries an absolute error of a few 2^-53.)"""
    Hm, Wm = shape
    P = Hm * Wm
    g = np.random.default_rng(7 + T)
    probs = g.uniform(0.05, 1.0, (1, T, 1 + P)).astype(np.float32)       # unnormalised on purpose
    exact = [[Fraction(float(v)) for v in probs[0, t]] for t in range(T)]
    for min_length in (0, 1, 2, T):
        want = [[Fraction(0)] * (2 * Wm - 1) for _ in range(2 * Hm - 1)]
        total = Fraction(0)
        for seq in itertools.product(range(1 + P), repeat=T):
            w = Fraction(1)
            for t, a in enumerate(seq):
                allowed = range(1, 1 + P) if t < min_length else range(1 + P)
                if a not in allowed:
                    w = Fraction(0)
                    break
                w *= exact[t][a] / sum(exact[t][k] for k in allowed)
            if not w:
                continue
            total += w
            fix = list(itertools.takewhile(lambda a: a != 0, seq))       # the first terminate ends the scanpath
            for a, b in zip(fix[:-1], fix[1:]):
                want[(b - 1) // Wm - (a - 1) // Wm + Hm - 1][(b - 1) % Wm - (a - 1) % Wm + Wm - 1] += w
        assert total == 1
        for max_steps in (1000, T):
            got = R.saccade_expectation(probs, [0], 1, shape, min_length, max_steps)
            assert got["bad"].tolist() == [0]
            for r in range(2 * Hm - 1):
                for c in range(2 * Wm - 1):
                    assert abs(got["E"][0, r, c] - float(want[r][c])) <= 1e-15, (min_length, r, c, got["E"][0, r, c], float(want[r][c]))
            assert abs(got["saccades"][0] - float(sum(sum(row) for row in want))) <= 1e-15
            assert abs(got["saccades"][0] - math.fsum(got["E"].reshape(-1).tolist())) <= 1e-15
        exactE, exact_total = R.row_expectation_exact(probs[0], shape, min_length, 1000)
        assert np.abs(exactE - np.array([[float(v) for v in row] for row in want])).max() <= 1e-16
        assert abs(exact_total - float(sum(sum(row) for row in want))) <= 1e-16
        wide, wide_total = R.row_expectation_wide(probs[0], shape, min_length, 1000)
        assert np.abs(wide - exactE).max() <= 1e-15 and abs(wide_total - exact_total) <= 1e-15


def test_restatement_rules_by_hand():
    # max_steps cuts the walk: Tm = 2 on uniform maps without terminate mass leaves ONE pair: every ordered cell pair has mass 1 / P^2
    shape, P = (2, 3), 6
    probs = np.full((3, 4, 1 + P), 0.5, dtype=np.float32)
    got = R.saccade_expectation(probs, [0, 2, 0], 2, shape, 4, 2)        # row 1: a group that does not exist
    want = np.array([[(2 - abs(dr)) * (3 - abs(dc)) for dc in range(-2, 3)] for dr in range(-1, 2)]) / 36.0
    assert got["bad"].tolist() == [0, -1, 0] and np.isnan(got["saccades"][1]) and got["saccades"][[0, 2]].tolist() == [1.0, 1.0]
    assert np.allclose(got["E"][0], 2 * want, rtol=0, atol=1e-15) and not got["E"][1].any()
    assert not R.saccade_expectation(probs, [0, 0, 0], 1, shape, 4, 1)["E"].any()            # Tm < 2: no pair
    assert R.saccade_expectation(probs, [0, 0, 0], 1, shape, 4, 1)["saccades"].tolist() == [0.0, 0.0, 0.0]
    # terminate mass: with p_0 = the cells' sum from min_length = 1 on, q = 1/2: saccade t survives (1/2)^(t+1) (q_0 = 0)
    got = R.saccade_expectation(np.concatenate([np.full((1, 4, 1), 3.0, np.float32), probs[:1, :, 1:]], 2), [0], 1, shape, 1, 1000)
    assert got["saccades"][0] == 0.5 + 0.25 + 0.125 and abs(got["E"].sum() - 0.875) <= 1e-15
    # a bad row: a zero step, NaN, inf -- only where t < Tm
    for value in (0.0, float("nan"), float("inf")):
        broken = probs.copy()
        broken[1, 2, 1:] = value if value == 0.0 else broken[1, 2, 1:]
        broken[1, 2, 3] = value
        got = R.saccade_expectation(broken, [0, 0, 1], 2, shape, 4, 1000)
        assert got["bad"].tolist() == [0, 1, 0] and np.isnan(got["saccades"][1]) and got["saccades"][0] == 3.0
        assert R.saccade_expectation(broken, [0, 0, 1], 2, shape, 4, 2)["bad"].tolist() == [0, 0, 0]       # t = 2 >= Tm: never read


def test_counts_restatement_by_hand():
    frame, shape = (30.0, 40.0), (3, 4)                                 # cells of 10 x 10 pixels
    nan = float("nan")
    paths = [np.array([(0.0, 0.0), (39.9, 29.9), (39.9, 29.9), (5.0, 15.0)]),             # (+2, +3), stay, (-1, -3)
             np.array([(5.0, 5.0), (40.0, 5.0), (15.0, 5.0), (15.0, 25.0)]),              # x = frame_w is outside: no bridging
             np.array([(nan, 1.0), (1.0, 1.0), (11.0, 1.0)]),
             np.zeros((0, 2)), np.array([(1.0, 1.0)])]
    res = R.saccade_counts(paths, [0, 0, 1, 1, 1], 3, frame, shape, 1000)
    assert res["saccades"].tolist() == [3, 1, 1, 0, 0] and res["dropped"].tolist() == [0, 1, 1, 0, 0]
    want = np.zeros((3, 5, 7), np.int64)
    want[0, 4, 6] = want[0, 2, 3] = want[0, 1, 0] = 1
    want[0, 4, 3] = 1                                                    # (15, 5) -> (15, 25): two rows down
    want[1, 2, 4] = 1
    assert np.array_equal(res["counts"], want)
    assert R.saccade_counts(paths, [0, 0, 1, 1, 1], 3, frame, shape, 2)["saccades"].tolist() == [1, 0, 0, 0, 0]
    assert R.saccade_counts([np.zeros((65, 2))], [0], 1, frame, shape, 5)["saccades"].tolist() == [-1]


# ---- the host statistics by hand -----------------------------------------------------------------------------------------------------------
FRAME, SHAPE = (30.0, 40.0), (3, 4)                                     # cells of 10 x 10 pixels; the lattice is 5 x 7, its centre [2, 3]
EDGES = [0.0, 5.0, 15.0, 25.0]


def _lattice(**entries):
    a = np.zeros((5, 7))
    for k, v in entries.items():
        dr, dc = (int(s.replace("m", "-")) for s in k.split("_")[1:])
        a[dr + 2, dc + 3] = v
    return a


def _both(lattice, n=4):
    got = M().saccade_summary(lattice, FRAME, amplitude_edges=EDGES, n_directions=n)
    want = R.summary(lattice, FRAME, EDGES, n)
    assert set(got) == {"total", "stay", "mean_amplitude", "amplitude_hist", "amplitude_overflow", "direction_hist"}
    for k in got:                   # sums of 35 non-negative terms in two orders: each within 35 * 2^-53 = 3.9e-15 relative of the true sum
        assert np.allclose(np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64), rtol=1e-14, atol=0, equal_nan=True), k
    return got


def test_lattice_vectors_and_sectors():
    dx, dy, amp = M().lattice_vectors(SHAPE, FRAME)
    assert dx.shape == dy.shape == amp.shape == (5, 7)
    assert dx[0].tolist() == [-30.0, -20.0, -10.0, 0.0, 10.0, 20.0, 30.0] and dy[:, 0].tolist() == [-20.0, -10.0, 0.0, 10.0, 20.0]
    assert amp[2, 3] == 0.0 and amp[2, 4] == 10.0 and amp[0, 3] == 20.0 and amp[4, 6] == math.sqrt(1300.0)
    dx, dy, amp = M().lattice_vectors((7, 9), (75, 100))                 # cells that are not square
    assert dx[6, 9] == 100.0 / 9 and dy[7, 8] == 75.0 / 7
    ref = R.vectors((7, 9), (75, 100))
    assert all(amp[dr + 6, dc + 8] == v[2] for (dr, dc), v in ref.items())
    sec = M().direction_sectors(SHAPE, FRAME, 4)                        # 0: right, 1: down (y points down), 2: left, 3: up
    assert sec[2, 3] == -1 and sec[2, 4] == 0 and sec[3, 3] == 1 and sec[2, 2] == 2 and sec[1, 3] == 3
    # exactly on a boundary (cells are square, so (+1, +1) lies at pi / 4): floor(atan2 * 4 / (2 pi) + 0.5) = floor(1.0) -> the sector
    # at the larger angle
    assert math.atan2(10.0, 10.0) * 4 / (2 * math.pi) + 0.5 == 1.0
    assert sec[3, 4] == 1 and sec[3, 2] == 2 and sec[1, 2] == 3 and sec[1, 4] == 0       # pi/4 -> 1, 3pi/4 -> 2, -3pi/4 -> 3 (-1 mod 4), -pi/4 -> 0
    assert sec[2, 0] == 2                                               # atan2 = pi: floor(2.5) = 2, not 4
    assert (M().direction_sectors(SHAPE, FRAME, 1)[sec >= 0] == 0).all()


def test_summary_by_hand():
    s = _both(_lattice(d_0_1=4.0))                                      # one-hot: one cell to the right, 10 pixels
    assert s["total"] == 4.0 and s["stay"] == 0.0 and s["mean_amplitude"] == 10.0
    assert s["amplitude_hist"].tolist() == [0.0, 1.0, 0.0] and s["amplitude_overflow"] == 0.0 and s["direction_hist"].tolist() == [1.0, 0.0, 0.0, 0.0]
    s = _both(_lattice(d_0_1=1.0, d_m2_0=3.0))                          # two-point: right 10 (1/4), up 20 (3/4)
    assert s["total"] == 4.0 and s["mean_amplitude"] == 17.5 and s["amplitude_hist"].tolist() == [0.0, 0.25, 0.75]
    assert s["direction_hist"].tolist() == [0.25, 0.0, 0.0, 0.75] and s["amplitude_overflow"] == 0.0
    s = _both(_lattice(d_0_0=5.0))                                      # stay-only: a direction needs a displacement
    assert s["stay"] == 1.0 and s["mean_amplitude"] == 0.0 and s["amplitude_hist"].tolist() == [1.0, 0.0, 0.0]
    assert np.isnan(s["direction_hist"]).all()
    s = _both(_lattice())                                               # empty
    assert s["total"] == 0.0 and np.isnan(s["stay"]) and np.isnan(s["mean_amplitude"]) and np.isnan(s["amplitude_overflow"])
    assert np.isnan(s["amplitude_hist"]).all() and np.isnan(s["direction_hist"]).all()
    s = _both(_lattice(d_1_1=2.0, d_0_0=2.0))                           # a vector on a sector boundary: sector 1; stays are left out
    assert s["direction_hist"].tolist() == [0.0, 1.0, 0.0, 0.0] and s["stay"] == 0.5
    s = _both(_lattice(d_0_3=1.0, d_2_0=1.0, d_0_1=2.0))                # 30 pixels: overflow; 20: the last bin; an edge value (15 is
    assert s["amplitude_overflow"] == 0.25 and s["amplitude_hist"].tolist() == [0.0, 0.5, 0.25]       # not hit) -- and 25 is exclusive:
    s25 = M().saccade_summary(_lattice(d_2_0=1.0), FRAME, amplitude_edges=[0.0, 20.0], n_directions=4)
    assert s25["amplitude_overflow"] == 1.0 and s25["amplitude_hist"].tolist() == [0.0]   # an amplitude AT the last edge overflows
    s10 = M().saccade_summary(_lattice(d_0_1=1.0), FRAME, amplitude_edges=[0.0, 10.0, 20.0], n_directions=4)
    assert s10["amplitude_hist"].tolist() == [0.0, 1.0]                  # half-open: [10, 20) holds 10
    below = M().saccade_summary(_lattice(d_0_0=1.0, d_0_1=1.0), FRAME, amplitude_edges=[5.0, 20.0], n_directions=4)
    assert below["amplitude_hist"].tolist() == [0.5] and below["amplitude_overflow"] == 0.0     # below the first edge: in no bin
    g = np.random.default_rng(3)                                        # integer counts and expectations alike, against the loops
    _both(g.integers(0, 9, (5, 7)), n=8)
    _both(g.uniform(0, 1, (5, 7)), n=3)


def test_jensen_shannon_and_wasserstein_by_hand():
    js, w1 = M().jensen_shannon, M().wasserstein_amplitude
    a, b = _lattice(d_0_1=2.0, d_1_0=6.0), _lattice(d_0_m1=5.0)
    assert js(a, a) == 0.0 and js(a, 3 * a) == 0.0 and js(a, b) == 1.0 and js(b, a) == 1.0
    assert np.isnan(js(a, _lattice())) and np.isnan(js(_lattice(), _lattice())) and np.isnan(js(a, _lattice(d_0_0=float("nan"))))
    p, q = [0.5, 0.5, 0.0], [0.0, 0.5, 0.5]                              # m = (1/4, 1/2, 1/4): 2 * 0.5 * (0.5 * log2 2) = 0.5
    assert js(p, q) == 0.5 == R.jensen_shannon(p, q)
    g = np.random.default_rng(5)
    x, y = g.uniform(0, 1, (5, 7)), g.integers(0, 4, (5, 7))
    assert abs(js(x, y) - R.jensen_shannon(x, y)) <= 1e-15 and 0.0 < js(x, y) < 1.0
    with pytest.raises(ValueError, match="equal shapes"):
        js([1.0, 2.0], [1.0])
    # W1: a distribution shifted by one cell width moves by that width; identical amplitudes in other directions cost nothing
    assert w1(_lattice(d_0_1=3.0), _lattice(d_0_2=1.0), FRAME) == 10.0
    assert w1(_lattice(d_0_1=1.0, d_0_2=1.0), _lattice(d_0_2=1.0, d_0_3=1.0), FRAME) == 10.0
    assert w1(_lattice(d_0_1=3.0), _lattice(d_m1_0=1.0), FRAME) == 0.0 and w1(a, a, FRAME) == 0.0
    assert w1(_lattice(d_0_0=1.0), _lattice(d_0_0=1.0, d_0_2=1.0), FRAME) == 10.0        # half of the mass moves 20 pixels
    assert np.isnan(w1(a, _lattice(), FRAME))
    assert abs(w1(x, y, FRAME) - R.wasserstein_amplitude(x, y, FRAME)) <= 1e-13
    with pytest.raises(ValueError, match="one shape"):
        w1(a, np.zeros((3, 3)), FRAME)
    cmp_ = M().saccade_comparison(a, b, FRAME, amplitude_edges=EDGES, n_directions=4)
    assert cmp_ == {"JSD_lattice": 1.0, "JSD_amplitude": 0.0, "JSD_direction": 1.0, "W1_amplitude": 0.0}    # both 10 pixels, other ways


def test_table_merges_sums_and_derives_from_the_summed_lattices():
    from scanpaths_amd.utils import evaluation as E
    g = np.random.default_rng(9)
    kw = dict(amplitude_edges=EDGES, n_directions=4)
    parts = [{"lattice_sum": g.integers(0, 5, (5, 7)), "human_lattice_sum": g.integers(0, 5, (5, 7)), "saccades_sum": 3, "scanpaths_count": 2,
              "fixations_dropped": 1, "rows_bad": 1, "summary": "not merged", "JSD_lattice": 0.3,
              "by_group": {"t": {"lattice_sum": g.integers(0, 5, (5, 7)), "saccades_sum": 1}}} for _ in range(3)]
    table = E.SaccadeStatisticsTable(FRAME, SHAPE, **kw)
    for p in parts:
        table.add(p)
    out = table.result()
    lat, hum = sum(p["lattice_sum"] for p in parts), sum(p["human_lattice_sum"] for p in parts)
    assert np.array_equal(out["lattice_sum"], lat) and out["lattice_sum"].dtype == np.int64 and out["saccades_sum"] == 9
    assert out["scanpaths_count"] == 6 and out["fixations_dropped"] == 3 and out["rows_bad"] == 3
    assert out["summary"]["total"] == float(lat.sum()) and out["human_summary"]["total"] == float(hum.sum())
    want = M().saccade_comparison(lat, hum, FRAME, **kw)
    assert all(out[k] == v for k, v in want.items())
    assert np.array_equal(out["by_group"]["t"]["lattice_sum"], sum(p["by_group"]["t"]["lattice_sum"] for p in parts))
    assert "JSD_lattice" not in out["by_group"]["t"] and out["by_group"]["t"]["summary"]["total"] > 0
    other = g.uniform(0, 1, (5, 7))
    no_human = E.SaccadeStatisticsTable(FRAME, SHAPE, **kw)
    no_human.add({"lattice_sum": parts[0]["lattice_sum"]})
    assert "JSD_lattice" not in no_human.result() and no_human.result(other)["JSD_lattice"] == M().jensen_shannon(parts[0]["lattice_sum"], other)
    assert parts[0]["lattice_sum"] is not no_human.parts["lattice_sum"]                      # add copies: the caller's array stays
    with pytest.raises(ValueError, match="the table's lattice"):
        no_human.add({"lattice_sum": np.zeros((3, 3))})
