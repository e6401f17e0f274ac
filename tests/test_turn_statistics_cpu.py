"""CPU-only checks of the turn-statistics layer: the three entry points are declared, bound and exported with equal
signatures and refuse bad arguments before any launch; every argument refusal of the Python layer is raised before a device or the
library is touched; the Python restatement of the closed form (tests/turn_statistics_ref.py) equals the exhaustive enumeration of all
action sequences under the sampler's rule in exact rational arithmetic -- which makes it independent of the closed form's own
reasoning -- and the host statistics hold answers worked out by hand."""
import inspect
import itertools
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import abi
import turn_statistics_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sp_scan_turn_max_directions": ("int", 0), "sp_scan_turn_counts": ("int", 18), "sp_scan_turn_expectation": ("int", 16)}


def M():
    from scanpaths_amd.utils.evaltools import turn_statistics
    return turn_statistics


def test_new_entry_points_are_declared_bound_and_exported():
    lib = abi.assert_declared(NEW, prefixes=("sp_scan_turn_",))
    assert not any(n.startswith("sp_scan_saccade_") for n in NEW)
    assert lib.sp_scan_turn_max_directions() == M().MAX_DIRECTIONS == R.MAX_DIRECTIONS == 16
    assert M().MAX_FIXATIONS == R.MAX_FIXATIONS == 64 and M().MAX_CELLS == R.MAX_CELLS == 2048
    assert "scanturn.hip" in open(os.path.join(ROOT, "scanpaths_amd", "csrc", "Makefile")).read()
    # the LDS limit is arithmetic: two bin arrays, three maps of 2048 cells and a sector table of D < 4 P bytes fit in 160 KB
    assert 2 * 17 * 256 * 8 + 3 * 2048 * 8 + 4 * 2048 <= 160 * 1024


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

    # sp_scan_turn_counts(fix, ncol, start, count, group, nscan, ngroups, max_steps, Hm, Wm, frame_w, frame_h, sector, n, counts, pairs, dropped, stream)
    ok = [p, 2, p, p, p, 5, 2, 6, 30, 40, 320.0, 240.0, p, 8, p, p, p, None]
    counts = lib.sp_scan_turn_counts
    for k in (0, 2, 3, 4, 12, 14, 15, 16):                          # inputs, the table and every output
        assert with_(counts, ok, **{f"a{k}": None}) == -2, k
    for k, bad in ((1, 1), (1, 0), (1, -2), (5, 0), (5, -1), (6, 0), (6, -1), (7, 0), (7, -3), (8, 0), (8, -30), (9, 0), (9, -1),
                   (8, 52), (9, 69), (8, 1 << 20), (10, 0.0), (10, -1.0), (10, nan), (10, inf), (11, 0.0), (11, -2.0), (11, nan), (11, inf),
                   (13, 0), (13, 17), (13, -1)):
        assert with_(counts, ok, **{f"a{k}": bad}) == -1, (k, bad)  # 52 x 40 = 2080 and 30 x 69 = 2070 cells: above 2048
    assert with_(counts, ok, a0=None, a1=1) == -2                   # NULL is answered before a bad scalar
    assert with_(counts, ok, a12=None, a13=0) == -2
    # sp_scan_turn_expectation(probs, row_group, R, T, Hm, Wm, ngroups, min_length, max_steps, sector, n, work, M, pairs, bad, stream)
    ok = [p, p, 3, 4, 30, 40, 2, 1, 6, p, 8, p, p, p, p, None]
    exp = lib.sp_scan_turn_expectation
    for k in (0, 1, 9, 11, 12, 13, 14):
        assert with_(exp, ok, **{f"a{k}": None}) == -2, k
    for k, bad in ((2, 0), (2, -1), (3, 0), (3, -2), (4, 0), (4, -30), (4, 52), (5, 0), (5, 69), (5, 1 << 20), (6, 0), (6, -1), (7, -1),
                   (8, 0), (8, -5), (10, 0), (10, 17), (10, -1)):
        assert with_(exp, ok, **{f"a{k}": bad}) == -1, (k, bad)
    assert with_(exp, ok, a1=None, a2=0) == -2                      # NULL is answered before a bad scalar
    assert with_(exp, ok, a11=None, a10=17) == -2
    assert with_(exp, ok, a4=32, a5=65) == -1                       # 2080 cells


def test_public_surface():
    from scanpaths_amd import inference
    from scanpaths_amd.utils import evaluation as E
    empty, KW = inspect.Parameter.empty, inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(M().turn_sectors).parameters
    assert list(p) == ["map_shape", "frame_size", "n_directions"] and all(v.default is empty for v in p.values())
    p = inspect.signature(M().turn_counts).parameters
    assert list(p) == ["scanpaths", "groups", "n_groups", "frame_size", "map_shape", "max_steps", "n_directions"]
    assert p["max_steps"].kind is KW and p["n_directions"].kind is KW and all(p[k].default is empty for k in p)
    p = inspect.signature(M().turn_expectation).parameters
    assert list(p) == ["probs", "row_groups", "n_groups", "min_length", "max_steps", "frame_size", "n_directions", "map_shape"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("min_length", "max_steps", "frame_size", "n_directions"))
    assert p["map_shape"].default is None
    assert list(inspect.signature(M().turn_summary).parameters) == ["table"]
    assert list(inspect.signature(M().turn_comparison).parameters) == ["table", "human_table"]
    p = inspect.signature(E.turn_statistics_evaluation).parameters
    assert list(p) == ["gt_fix_vectors", "predict_fix_vectors", "gt_keys", "predict_keys", "frame_size", "map_shape", "max_steps",
                       "n_directions", "groups", "image_keys"]
    assert all(p[k].kind is KW and p[k].default is empty for k in list(p)[4:8]) and p["groups"].default is None
    p = inspect.signature(E.turn_statistics_human_evaluation).parameters
    assert list(p) == ["gt_fix_vectors", "gt_keys", "frame_size", "map_shape", "max_steps", "n_directions", "groups", "image_keys"]
    p = inspect.signature(E.turn_statistics_model_evaluation).parameters
    assert list(p) == ["predict", "keys", "min_length", "max_steps", "n_directions", "performances", "frame_size", "map_shape", "groups",
                       "human_table"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("min_length", "max_steps", "n_directions"))
    assert list(inspect.signature(E.TurnStatisticsTable.__init__).parameters) == ["self", "n_directions"]
    assert list(inspect.signature(E.TurnStatisticsTable.result).parameters) == ["self", "human_table"]
    assert issubclass(E.TurnStatisticsTable, E._SumTable)
    p = inspect.signature(inference.run_turn_statistics_loop).parameters
    assert list(p) == ["model", "loader", "min_length", "max_steps", "n_directions", "human_table", "ablate_attention_info", "frame_size",
                       "map_shape"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("min_length", "max_steps", "n_directions"))
    # the saccade-statistics counterparts stay as they were
    assert list(inspect.signature(E.SaccadeStatisticsTable.result).parameters) == ["self", "human_lattice"]
    assert list(inspect.signature(E.saccade_statistics_model_evaluation).parameters)[:4] == ["predict", "keys", "min_length", "max_steps"]


def test_refusals_come_before_any_device_call(monkeypatch):
    from scanpaths_amd import hip, inference
    from scanpaths_amd.utils import evaluation as E

    def no_lib():
        raise AssertionError("validation must come first")

    monkeypatch.setattr(M(), "_device", no_lib)
    monkeypatch.setattr(hip, "lib", no_lib)
    sp = np.array([[1.0, 1.0, 0.2], [5.0, 3.0, 0.3], [9.0, 3.0, 0.3]])
    frame, shape = (24, 40), (3, 5)
    counts = M().turn_counts
    with pytest.raises(TypeError):
        counts([sp], [0], 1, frame, shape, n_directions=4)                                  # max_steps has no default
    with pytest.raises(TypeError):
        counts([sp], [0], 1, frame, shape, max_steps=6)                                     # nor has n_directions
    for bad in (0, -1, 1.5, True, None):
        with pytest.raises(ValueError, match="max_steps"):
            counts([sp], [0], 1, frame, shape, max_steps=bad, n_directions=4)
    for bad in (0, -1, 2.5, None, True, 17):
        with pytest.raises(ValueError, match="n_directions"):
            counts([sp], [0], 1, frame, shape, max_steps=6, n_directions=bad)
    with pytest.raises(ValueError, match="kernel limit"):
        counts([np.zeros((M().MAX_FIXATIONS + 1, 2))], [0], 1, frame, shape, max_steps=6, n_directions=4)
    for bad in ((0, 5), (3,), (3, -5), (2.5, 4), None, (3, 5, 7)):
        with pytest.raises(ValueError, match="map_shape"):
            counts([sp], [0], 1, frame, bad, max_steps=6, n_directions=4)
    with pytest.raises(ValueError, match="kernel limit"):
        counts([sp], [0], 1, frame, (32, 65), max_steps=6, n_directions=4)                  # 2080 cells
    for bad in ([1], [-1], [2]):
        with pytest.raises(ValueError, match="out of range"):
            counts([sp], bad, 1, frame, shape, max_steps=6, n_directions=4)
    with pytest.raises(ValueError, match="one group per scanpath"):
        counts([sp, sp], [0], 1, frame, shape, max_steps=6, n_directions=4)
    for bad in (0, -1, None, 1.5):
        with pytest.raises(ValueError, match="n_groups"):
            counts([sp], [0], bad, frame, shape, max_steps=6, n_directions=4)
    for bad in ((0, 32), (24, float("inf")), (float("nan"), 32)):
        with pytest.raises(ValueError, match="frame_size"):
            counts([sp], [0], 1, bad, shape, max_steps=6, n_directions=4)
    with pytest.raises(ValueError, match="scanpath is an"):
        counts([np.zeros((3, 1))], [0], 1, frame, shape, max_steps=6, n_directions=4)
    res = counts([], [], 2, frame, shape, max_steps=3, n_directions=4)                      # nothing to count: zeros, no device
    assert res["counts"].dtype == np.int64 and res["counts"].shape == (2, 5, 5) and not res["counts"].any()
    assert res["pairs"].dtype == res["dropped"].dtype == np.int32 and res["pairs"].shape == (0,)
    for bad in (0, 17, None):
        with pytest.raises(ValueError, match="n_directions"):
            M().turn_sectors(shape, frame, bad)

    T = 4
    probs = torch.full((2, T, 16), 1.0 / 16)
    exp = M().turn_expectation
    ok = dict(min_length=1, max_steps=4, frame_size=frame, n_directions=4, map_shape=shape)
    for missing in ("min_length", "max_steps", "frame_size", "n_directions"):
        with pytest.raises(TypeError):
            exp(probs, [0, 0], 1, **{k: v for k, v in ok.items() if k != missing})
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="min_length"):
            exp(probs, [0, 0], 1, **dict(ok, min_length=bad))
    for bad in (0, 2.5, None):
        with pytest.raises(ValueError, match="max_steps"):
            exp(probs, [0, 0], 1, **dict(ok, max_steps=bad))
    for bad in (0, 17, -1, None, 2.5):
        with pytest.raises(ValueError, match="n_directions"):
            exp(probs, [0, 0], 1, **dict(ok, n_directions=bad))
    for bad in ((0, 32), (24, float("inf"))):
        with pytest.raises(ValueError, match="frame_size"):
            exp(probs, [0, 0], 1, **dict(ok, frame_size=bad))
    with pytest.raises(ValueError, match="probs"):
        exp(probs[0], [0, 0], 1, **ok)
    with pytest.raises(ValueError, match="probs"):
        exp(probs.numpy(), [0, 0], 1, **ok)
    with pytest.raises(ValueError, match="map_shape is required"):
        exp(probs, [0, 0], 1, **dict(ok, map_shape=None))
    for bad in ((4, 4), (3, 6), (0, 15), (-3, -5)):
        with pytest.raises(ValueError, match="map_shape"):
            exp(probs, [0, 0], 1, **dict(ok, map_shape=bad))
    with pytest.raises(ValueError, match="kernel limit"):
        exp(torch.zeros(1, 2, 2081), [0], 1, **dict(ok, map_shape=(32, 65)))
    for bad in ([0, 1], [-1, 0]):
        with pytest.raises(ValueError, match="out of range"):
            exp(probs, bad, 1, **ok)
    with pytest.raises(ValueError, match="one group per row"):
        exp(probs, [0], 1, **ok)
    for bad in (np.zeros((3, 4)), np.zeros(9), np.zeros((1, 1))):
        with pytest.raises(ValueError, match="transition table"):
            M().turn_summary(bad)
    with pytest.raises(ValueError, match="one shape"):
        M().turn_comparison(np.ones((5, 5)), np.ones((9, 9)))

    # the keyed layer
    ev = E.turn_statistics_evaluation
    kw = dict(frame_size=frame, map_shape=shape, max_steps=3, n_directions=4)
    for missing in kw:
        with pytest.raises(TypeError):
            ev([sp], [sp], ["a"], ["a"], **{k: v for k, v in kw.items() if k != missing})
    with pytest.raises(ValueError, match="n_directions"):
        ev([sp], [sp], ["a"], ["a"], **dict(kw, n_directions=17))
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
    mv = E.turn_statistics_model_evaluation
    mkw = dict(min_length=1, max_steps=3, n_directions=4, frame_size=frame, map_shape=shape)
    for missing in ("min_length", "max_steps", "n_directions"):
        with pytest.raises(TypeError):
            mv(one, ["a", "b"], **{k: v for k, v in mkw.items() if k != missing})
    with pytest.raises(ValueError, match="predict lacks 'good_all_actions_prob'"):
        mv(one, ["a", "b"], performances=[[True], [False]], **mkw)
    with pytest.raises(ValueError, match="predict lacks 'all_actions_prob'"):
        mv(two, ["a", "b"], **mkw)
    with pytest.raises(ValueError, match="one list of performances per sample"):
        mv(two, ["a", "b"], performances=[[True]], **mkw)
    with pytest.raises(ValueError, match="samples"):
        mv(one, ["a", "b", "a"], **mkw)
    with pytest.raises(ValueError, match="map_shape"):
        mv(one, ["a", "b"], **dict(mkw, map_shape=None))
    with pytest.raises(ValueError, match="human_table"):
        mv(one, ["a", "b"], human_table=np.ones((9, 9)), **mkw)
    with pytest.raises(ValueError, match="has no group"):
        mv(one, ["a", "b"], groups={"a": 0}, **mkw)
    for bad in (0, 17):
        with pytest.raises(ValueError, match="n_directions"):
            E.TurnStatisticsTable(bad)
        with pytest.raises(ValueError, match="n_directions"):
            inference.run_turn_statistics_loop(None, [], min_length=1, max_steps=3, n_directions=bad)


def test_no_cpu_path(monkeypatch):
    from scanpaths_amd import hip
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(hip.HipError, match="no CPU path"):
        M().turn_counts([np.array([[1.0, 1.0]])], [0], 1, (24, 32), (3, 4), max_steps=2, n_directions=4)
    with pytest.raises(hip.HipError, match="no CPU path"):
        M().turn_expectation(torch.zeros(1, 2, 13), [0], 1, min_length=0, max_steps=2, frame_size=(24, 32), n_directions=4, map_shape=(3, 4))


# ---- the sector table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,frame,n", [((3, 4), (30.0, 40.0), 4), ((7, 9), (100.0, 300.0), 8), ((1, 1), (75.0, 100.0), 1),
                                           ((1, 3), (75.0, 100.0), 2), ((2, 2), (75.0, 100.0), 3), ((30, 40), (240, 320), 16)])
def test_turn_sectors_agree_with_direction_sectors(shape, frame, n):
    from scanpaths_amd.utils.evaltools.saccade_statistics import direction_sectors
    Hm, Wm = shape
    sec, old = M().turn_sectors(shape, frame, n), direction_sectors(shape, frame, n)
    assert sec.dtype == np.int32 and sec.shape == (2 * Hm - 1, 2 * Wm - 1) and sec.flags["C_CONTIGUOUS"]
    assert sec[Hm - 1, Wm - 1] == n and old[Hm - 1, Wm - 1] == -1 and (old == -1).sum() == 1
    assert np.array_equal(np.where(old < 0, n, old), sec) and sec.min() >= 0 and sec.max() <= n
    # the entry of (dr, dc) sits at (dr + Hm - 1) * (2 Wm - 1) + dc + Wm - 1 of the flat table the kernels read
    flat = sec.reshape(-1)
    for dr, dc in ((0, 0), (Hm - 1, Wm - 1), (-(Hm - 1), 0), (0, -(Wm - 1))):
        assert flat[(dr + Hm - 1) * (2 * Wm - 1) + dc + Wm - 1] == sec[dr + Hm - 1, dc + Wm - 1]
    if shape[0] * shape[1] <= 64:
        assert np.array_equal(sec, R.sectors(shape, frame, n))           # the loop with math.atan2
    if shape == (3, 4):                                                  # 0: right, 1: down (y points down), 2: left, 3: up; square cells
        assert sec[2, 4] == 0 and sec[3, 3] == 1 and sec[2, 2] == 2 and sec[1, 3] == 3 and sec[3, 4] == 1      # pi / 4 -> the larger angle


# ---- the restatement against exhaustive enumeration ------------------------------------------------------------------------------------
CASES = [((2, 2), 4, 4, 0, 4), ((2, 2), 4, 3, 2, 4), ((1, 3), 4, 2, 1, 3), ((2, 2), 4, 8, 5, 4), ((2, 3), 3, 5, 1, 3), ((2, 2), 4, 4, 4, 4)]


@pytest.mark.parametrize("shape,T,n,min_length,max_steps", CASES)
def test_restatement_equals_the_exhaustive_enumeration(shape, T, n, min_length, max_steps):
    """All (1 + P)^T action sequences under the sampler's rule (terminate masked for t < min_length, the first terminate ends the
    scanpath; only the first max_steps fixations count), weighted in exact rationals: the expected number of saccade pairs per (k, k'),
    entry by entry, to 1e-15 absolute; "pairs" equals the table's total.  (Every entry is a sum of non-negative terms that add up to at
    most T - 2 <= 2; a double sum of so few terms carries an absolute error of a few 2^-53.)"""
    Hm, Wm = shape
    P = Hm * Wm
    frame = (75.0, 100.0)
    sector = R.sectors(shape, frame, n)
    g = np.random.default_rng(11 * T + P + n)
    probs = g.uniform(0.05, 1.0, (1, T, 1 + P)).astype(np.float32)       # unnormalised on purpose
    exact = [[Fraction(float(v)) for v in probs[0, t]] for t in range(T)]
    want = [[Fraction(0)] * (n + 1) for _ in range(n + 1)]
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
        fix = list(itertools.takewhile(lambda a: a != 0, seq))[:max_steps]   # the first terminate ends the scanpath
        cells = [((a - 1) // Wm, (a - 1) % Wm) for a in fix]
        for a, b, c in zip(cells[:-2], cells[1:-1], cells[2:]):
            want[sector[b[0] - a[0] + Hm - 1, b[1] - a[1] + Wm - 1]][sector[c[0] - b[0] + Hm - 1, c[1] - b[1] + Wm - 1]] += w
    assert total == 1
    wantf = np.array([[float(v) for v in row] for row in want])
    assert wantf.sum() > 0.1
    got = R.turn_expectation(probs, [0], 1, sector, min_length, max_steps)
    assert got["bad"].tolist() == [0]
    assert np.abs(got["M"][0] - wantf).max() <= 1e-15, (got["M"][0], wantf)
    assert abs(got["pairs"][0] - float(sum(sum(row) for row in want))) <= 1e-15
    exactM, exact_total = R.row_expectation_exact(probs[0], sector, min_length, max_steps)
    assert np.abs(exactM - wantf).max() <= 1e-16 and abs(exact_total - float(sum(sum(row) for row in want))) <= 1e-16
    wide, wide_total = R.row_expectation_wide(probs[0], sector, min_length, max_steps)
    assert np.abs(wide - exactM).max() <= 1e-15 and abs(wide_total - exact_total) <= 1e-15
    for doubles in (True,):
        again, _ = R.row_expectation_exact(probs[0], sector, min_length, max_steps, doubles=doubles)
        assert np.abs(again - wantf).max() <= 1e-15


def test_restatement_rules_by_hand():
    # uniform maps without terminate mass, Tm = 3: ONE triple; every ordered cell triple has mass 1 / P^3
    shape, P, n = (2, 3), 6, 4
    sector = R.sectors(shape, (20.0, 30.0), n)
    probs = np.full((3, 4, 1 + P), 0.5, dtype=np.float32)
    got = R.turn_expectation(probs, [0, 2, 0], 2, sector, 4, 3)          # row 1: a group that does not exist
    want = np.zeros((n + 1, n + 1))
    for a, b, c in itertools.product(range(P), repeat=3):
        want[sector[b // 3 - a // 3 + 1, b % 3 - a % 3 + 2], sector[c // 3 - b // 3 + 1, c % 3 - b % 3 + 2]] += 1.0 / P ** 3
    assert got["bad"].tolist() == [0, -1, 0] and np.isnan(got["pairs"][1]) and got["pairs"][[0, 2]].tolist() == [1.0, 1.0]
    assert np.allclose(got["M"][0], 2 * want, rtol=0, atol=1e-15) and not got["M"][1].any()
    for Tm in (1, 2):                                                    # Tm < 3: no pair
        assert not R.turn_expectation(probs, [0, 0, 0], 1, sector, 4, Tm)["M"].any()
        assert R.turn_expectation(probs, [0, 0, 0], 1, sector, 4, Tm)["pairs"].tolist() == [0.0, 0.0, 0.0]
    # terminate mass: with p_0 = the cells' sum from min_length = 1 on, q = 1/2: pair t survives (1/2)^(t+2) (q_0 = 0)
    got = R.turn_expectation(np.concatenate([np.full((1, 4, 1), 3.0, np.float32), probs[:1, :, 1:]], 2), [0], 1, sector, 1, 1000)
    assert got["pairs"][0] == 0.25 + 0.125 and abs(got["M"].sum() - 0.375) <= 1e-15
    # a bad row: a zero step, NaN, inf -- only where t < Tm
    for value in (0.0, float("nan"), float("inf")):
        broken = probs.copy()
        broken[1, 3, 1:] = value if value == 0.0 else broken[1, 3, 1:]
        broken[1, 3, 3] = value
        got = R.turn_expectation(broken, [0, 0, 1], 2, sector, 4, 1000)
        assert got["bad"].tolist() == [0, 1, 0] and np.isnan(got["pairs"][1]) and got["pairs"][0] == 2.0
        assert R.turn_expectation(broken, [0, 0, 1], 2, sector, 4, 3)["bad"].tolist() == [0, 0, 0]         # t = 3 >= Tm: never read


def test_counts_restatement_by_hand():
    frame, shape, n = (30.0, 40.0), (3, 4), 4                           # cells of 10 x 10 pixels; 0 right, 1 down, 2 left, 3 up, 4 stay
    sector = R.sectors(shape, frame, n)
    nan = float("nan")
    paths = [np.array([(5.0, 5.0), (25.0, 5.0), (35.0, 5.0), (35.0, 5.0), (15.0, 5.0), (15.0, 25.0)]),   # right right stay left down
             np.array([(5.0, 5.0), (15.0, 5.0), (40.0, 5.0), (15.0, 5.0), (25.0, 5.0), (35.0, 5.0)]),    # x = frame_w is outside
             np.array([(nan, 1.0), (1.0, 1.0), (11.0, 1.0), (1.0, 1.0)]),
             np.zeros((0, 2)), np.array([(1.0, 1.0)]), np.array([(1.0, 1.0), (11.0, 1.0)])]
    res = R.turn_counts(paths, [0, 0, 1, 1, 1, 1], 3, frame, shape, 1000, sector)
    assert res["pairs"].tolist() == [4, 1, 1, 0, 0, 0] and res["dropped"].tolist() == [0, 1, 1, 0, 0, 0]
    want = np.zeros((3, 5, 5), np.int64)
    want[0, 0, 0] = 2                                                    # right -> right, in both scanpaths of group 0
    want[0, 0, 4] = want[0, 4, 2] = want[0, 2, 1] = 1
    want[1, 0, 2] = 1                                                    # right, then back: a reversal
    assert np.array_equal(res["counts"], want)
    assert R.turn_counts(paths, [0, 0, 1, 1, 1, 1], 3, frame, shape, 3, sector)["pairs"].tolist() == [1, 0, 0, 0, 0, 0]
    assert R.turn_counts([np.zeros((65, 2))], [0], 1, frame, shape, 5, sector)["pairs"].tolist() == [-1]


# ---- the host statistics by hand -----------------------------------------------------------------------------------------------------------
def _both(table):
    got, want = M().turn_summary(table), R.summary(table)
    assert set(got) == {"total", "moving", "turn_hist", "forward", "reversal", "persistence", "stay_then_move", "move_then_stay",
                        "stay_then_stay", "transition"} == set(want)
    for k in got:                   # sums of at most 17^2 non-negative terms in two orders; the cosine sum is bounded by the shares' sum 1
        assert np.allclose(np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64), rtol=1e-13, atol=1e-15,
                           equal_nan=True), k
    return got


def test_summary_by_hand():
    t = np.zeros((5, 5))
    t[np.arange(4), np.arange(4)] = [1.0, 2.0, 3.0, 4.0]                # all forward
    s = _both(t)
    assert s["total"] == s["moving"] == 10.0 and s["turn_hist"].tolist() == [1.0, 0.0, 0.0, 0.0] and s["forward"] == 1.0
    assert s["reversal"] == 0.0 and s["persistence"] == 1.0 and s["stay_then_move"] == s["move_then_stay"] == s["stay_then_stay"] == 0.0
    assert np.array_equal(s["transition"], t[:4, :4] / 10.0)
    t = np.zeros((5, 5))
    t[0, 2], t[1, 3], t[2, 0], t[3, 1] = 1.0, 1.0, 2.0, 4.0              # all reversal, n = 4
    s = _both(t)
    assert s["turn_hist"].tolist() == [0.0, 0.0, 1.0, 0.0] and s["reversal"] == 1.0 and s["forward"] == 0.0 and s["persistence"] == -1.0
    t = np.zeros((4, 4))                                                # odd n: no sector is opposite
    t[0, 1], t[1, 2], t[2, 0], t[0, 0] = 1.0, 1.0, 1.0, 1.0              # three turns of one sector, one forward
    s = _both(t)
    assert s["turn_hist"].tolist() == [0.25, 0.75, 0.0] and np.isnan(s["reversal"]) and s["forward"] == 0.25
    assert abs(s["persistence"] - (0.25 + 0.75 * np.cos(2 * np.pi / 3))) <= 1e-15
    t = np.zeros((5, 5))
    t[4, 4] = 3.0                                                       # stay-only
    s = _both(t)
    assert s["total"] == 3.0 and s["moving"] == 0.0 and s["stay_then_stay"] == 1.0 and s["stay_then_move"] == 0.0
    assert np.isnan(s["turn_hist"]).all() and np.isnan(s["forward"]) and np.isnan(s["reversal"]) and np.isnan(s["persistence"])
    assert np.isnan(s["transition"]).all() and s["transition"].shape == (4, 4)
    s = _both(np.zeros((9, 9)))                                         # empty
    assert s["total"] == 0.0 and all(np.isnan(s[k]) for k in ("stay_then_move", "move_then_stay", "stay_then_stay", "forward", "persistence"))
    assert np.isnan(s["turn_hist"]).all() and s["turn_hist"].shape == (8,)
    t = np.zeros((5, 5))
    t[0, 1], t[4, 0], t[2, 4], t[4, 4] = 2.0, 1.0, 3.0, 2.0              # mixed: the shares are of total, the histogram of moving
    s = _both(t)
    assert s["total"] == 8.0 and s["moving"] == 2.0 and s["stay_then_move"] == 0.125 and s["move_then_stay"] == 0.375
    assert s["stay_then_stay"] == 0.25 and s["turn_hist"].tolist() == [0.0, 1.0, 0.0, 0.0]
    g = np.random.default_rng(3)                                        # integer counts and expectations alike, against the loops
    _both(g.integers(0, 9, (9, 9)))
    _both(g.uniform(0, 1, (17, 17)))
    _both(g.uniform(0, 1, (2, 2)))                                      # n = 1: every moving pair is "forward"
    # the comparison: identical shares 0, disjoint ones 1 bit
    a, b = np.zeros((5, 5)), np.zeros((5, 5))
    a[0, 0], b[0, 2] = 2.0, 5.0
    assert M().turn_comparison(a, 3 * a) == {"JSD_turn": 0.0, "JSD_transition": 0.0}
    assert M().turn_comparison(a, b) == {"JSD_turn": 1.0, "JSD_transition": 1.0}
    b[0, 2], b[1, 1] = 0.0, 1.0                                         # forward both, other sectors: the histograms agree, the tables do not
    assert M().turn_comparison(a, b) == {"JSD_turn": 0.0, "JSD_transition": 1.0}
    x, y = g.uniform(0, 1, (9, 9)), g.integers(0, 4, (9, 9))
    c = M().turn_comparison(x, y)
    assert abs(c["JSD_transition"] - R.jensen_shannon(x[:8, :8], y[:8, :8])) <= 1e-15
    assert abs(c["JSD_turn"] - R.jensen_shannon(R.summary(x)["turn_hist"], R.summary(y)["turn_hist"])) <= 1e-15
    assert np.isnan(M().turn_comparison(a, np.zeros((5, 5)))["JSD_turn"])


def test_table_merges_sums_and_derives_from_the_summed_tables():
    from scanpaths_amd.utils import evaluation as E
    g = np.random.default_rng(9)
    parts = [{"table_sum": g.integers(0, 5, (5, 5)), "human_table_sum": g.integers(0, 5, (5, 5)), "pairs_sum": 3, "scanpaths_count": 2,
              "fixations_dropped": 1, "rows_bad": 1, "summary": "not merged", "JSD_turn": 0.3,
              "by_group": {"t": {"table_sum": g.integers(0, 5, (5, 5)), "pairs_sum": 1}}} for _ in range(3)]
    table = E.TurnStatisticsTable(4)
    for p in parts:
        table.add(p)
    out = table.result()
    tab, hum = sum(p["table_sum"] for p in parts), sum(p["human_table_sum"] for p in parts)
    assert np.array_equal(out["table_sum"], tab) and out["table_sum"].dtype == np.int64 and out["pairs_sum"] == 9      # integers: exact
    assert out["scanpaths_count"] == 6 and out["fixations_dropped"] == 3 and out["rows_bad"] == 3
    assert out["summary"]["total"] == float(tab.sum()) and out["human_summary"]["total"] == float(hum.sum())
    assert all(out[k] == v for k, v in M().turn_comparison(tab, hum).items())
    assert np.array_equal(out["by_group"]["t"]["table_sum"], sum(p["by_group"]["t"]["table_sum"] for p in parts))
    assert "JSD_turn" not in out["by_group"]["t"] and out["by_group"]["t"]["summary"]["total"] > 0
    other = g.uniform(0, 1, (5, 5))
    no_human = E.TurnStatisticsTable(4)
    no_human.add({"table_sum": parts[0]["table_sum"]})
    assert "JSD_turn" not in no_human.result()
    assert no_human.result(other)["JSD_transition"] == M().jensen_shannon(parts[0]["table_sum"][:4, :4], other[:4, :4])
    assert parts[0]["table_sum"] is not no_human.parts["table_sum"]                          # add copies: the caller's array stays
    with pytest.raises(ValueError, match="the table's lattice"):
        no_human.add({"table_sum": np.zeros((9, 9))})
    # expectations: two halves merged equal one sum over the union to 1e-13 relative -- every term is non-negative and only a handful of
    # additions are re-associated ((a + b) + (c + d) against ((a + b) + c) + d: each side within 3 * 2^-53 relative of the true sum)
    rows = [g.uniform(0, 1, (5, 5)) for _ in range(4)]
    halves = E.TurnStatisticsTable(4)
    halves.add({"table_sum": rows[0] + rows[1], "pairs_sum": float((rows[0] + rows[1]).sum()), "rows_count": 2})
    halves.add({"table_sum": rows[2] + rows[3], "pairs_sum": float((rows[2] + rows[3]).sum()), "rows_count": 2})
    union = ((rows[0] + rows[1]) + rows[2]) + rows[3]
    merged = halves.result()
    assert merged["rows_count"] == 4 and np.allclose(merged["table_sum"], union, rtol=1e-13, atol=0)
    assert abs(merged["pairs_sum"] - union.sum()) <= 1e-13 * union.sum()
