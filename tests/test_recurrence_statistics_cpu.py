"""CPU-only checks of the recurrence-statistics layer: the second library's header, binding and exports name the same
functions and leave the main library's 154 entry points alone; its launchers refuse bad arguments before any launch; every argument
refusal of the Python layer is raised before a device or a library is touched; the mask, the RQA integers, the four measures, the
summary, the comparison and the table hold answers worked out by hand; and the Python restatement of the closed form
(tests/recurrence_statistics_ref.py) equals the exhaustive enumeration of all action sequences under the sampler's rule in exact
rational arithmetic -- which makes it independent of the closed form's own reasoning."""
import inspect
import itertools
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import abi
import recurrence_statistics_ref as R
import stats_abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"sp_stats_abi_version": ("int", 0), "sp_stats_max_fixations": ("int", 0), "sp_stats_max_cells": ("int", 0),
       "sp_stats_recurrence_counts": ("int", 19), "sp_stats_recurrence_expectation": ("int", 15)}


def M():
    from scanpaths_amd.utils.evaltools import recurrence_statistics
    return recurrence_statistics


# ---- the second library -------------------------------------------------------------------------------------------------------------------
def test_stats_header_binding_and_exports_agree():
    from scanpaths_amd import hip
    decls = stats_abi.header_decls()
    assert set(decls) == set(NEW) == set(hip.STATS_SIGNATURES) == set(stats_abi.exported_functions(stats_abi.lib_path()))
    for name, (ret, nargs) in NEW.items():
        assert decls[name][0] == ret and len(decls[name][1]) == nargs, (name, decls[name])
        cret, cargs = hip.STATS_SIGNATURES[name]
        assert cret is stats_abi.KINDS[ret] and len(cargs) == nargs, (name, cret, cargs)
        for a, c in zip(decls[name][1], cargs):
            assert c is stats_abi.want_ctype(a), (name, a, c)
    lib = stats_abi.raw_lib()
    assert stats_abi.header_version() == hip.STATS_ABI_VERSION == lib.sp_stats_abi_version() == 1
    assert lib.sp_stats_max_fixations() == M().MAX_FIXATIONS == R.MAX_FIXATIONS == 64
    assert lib.sp_stats_max_cells() == M().MAX_CELLS == R.MAX_CELLS == 2048
    makefile = open(os.path.join(ROOT, "scanpaths_amd", "csrc", "Makefile")).read()
    assert "scanrecur.hip" in makefile and "all: $(OUT) $(STATS_OUT)" in makefile
    assert "scanrecur.hip" not in [w for line in makefile.splitlines() if line.startswith("SRCS") for w in line.split()]
    # the LDS of the closed form is arithmetic: two maps of 2048 cells in double, three arrays of 64 doubles and 64 flags, under 64 KB
    assert 2 * 2048 * 8 + 3 * 64 * 8 + 64 * 4 <= 64 * 1024


def test_main_library_is_untouched():
    from scanpaths_amd import hip
    assert len(hip.SIGNATURES) == 154 and hip.ABI_VERSION == abi.header_abi_version() == 4
    main, stats = set(abi.exported_functions()), set(stats_abi.exported_functions(stats_abi.lib_path()))
    assert len(main) == 154 and not main & stats and not set(hip.SIGNATURES) & set(hip.STATS_SIGNATURES)
    assert not set(abi.header_symbols()) & set(stats_abi.header_decls())


def test_stats_lib_loads_once_and_refuses_a_missing_or_mismatched_library(monkeypatch, tmp_path):
    from scanpaths_amd import hip
    stats_abi.lib_path()
    first = hip.stats_lib()
    assert hip.stats_lib() is first and first.sp_stats_recurrence_counts.argtypes == hip.STATS_SIGNATURES["sp_stats_recurrence_counts"][1]
    monkeypatch.setattr(hip, "_stats_lib", None)
    monkeypatch.setattr(hip, "STATS_LIB_PATH", str(tmp_path / "libscanpaths_amd_stats.so"))
    with pytest.raises(RuntimeError, match=r"is missing: build it with .*g\.build\(\)"):
        hip.stats_lib()
    monkeypatch.undo()
    monkeypatch.setattr(hip, "_stats_lib", None)
    monkeypatch.setattr(hip, "STATS_ABI_VERSION", 2)
    with pytest.raises(RuntimeError, match="ABI version 1, this binding expects 2"):
        hip.stats_lib()
    monkeypatch.undo()
    assert hip.stats_lib() is first


def test_launchers_refuse_bad_arguments_without_a_device():
    """SP_ENULL (-2) / SP_EINVAL (-1) come before the launch, so on a machine without a GPU too.  Every call below is a refused one."""
    lib = stats_abi.raw_lib()
    p = 4096                                                        # any non-NULL value: nothing is dereferenced before the checks
    nan, inf = float("nan"), float("inf")

    def with_(call, base, **kw):
        a = list(base)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)

    # (fix, ncol, start, count, group, nscan, ngroups, max_steps, Hm, Wm, frame_w, frame_h, mask, min_line, counts, points, dropped, rqa, stream)
    ok = [p, 2, p, p, p, 5, 2, 6, 30, 40, 320.0, 240.0, p, 2, p, p, p, p, None]
    counts = lib.sp_stats_recurrence_counts
    for k in (0, 2, 3, 4, 12, 14, 15, 16, 17):                      # inputs, the mask and every output
        assert with_(counts, ok, **{f"a{k}": None}) == -2, k
    for k, bad in ((1, 1), (1, 0), (1, -2), (5, 0), (5, -1), (6, 0), (6, -1), (7, 0), (7, -3), (7, 65), (8, 0), (8, -30), (9, 0), (9, -1),
                   (8, 52), (9, 69), (8, 1 << 20), (10, 0.0), (10, -1.0), (10, nan), (10, inf), (11, 0.0), (11, -2.0), (11, nan), (11, inf),
                   (13, 1), (13, 0), (13, -2)):
        assert with_(counts, ok, **{f"a{k}": bad}) == -1, (k, bad)  # 52 x 40 = 2080 and 30 x 69 = 2070 cells: above 2048
    assert with_(counts, ok, a0=None, a1=1) == -2                   # NULL is answered before a bad scalar
    assert with_(counts, ok, a17=None, a13=0) == -2
    # (probs, row_group, R, T, Hm, Wm, ngroups, min_length, max_steps, mask, work, E, points, bad, stream)
    ok = [p, p, 3, 4, 30, 40, 2, 1, 6, p, p, p, p, p, None]
    exp = lib.sp_stats_recurrence_expectation
    for k in (0, 1, 9, 10, 11, 12, 13):
        assert with_(exp, ok, **{f"a{k}": None}) == -2, k
    for k, bad in ((2, 0), (2, -1), (3, 0), (3, -2), (4, 0), (4, -30), (4, 52), (5, 0), (5, 69), (5, 1 << 20), (6, 0), (6, -1), (7, -1),
                   (8, 0), (8, -5), (8, 65)):
        assert with_(exp, ok, **{f"a{k}": bad}) == -1, (k, bad)
    assert with_(exp, ok, a1=None, a2=0) == -2                      # NULL is answered before a bad scalar
    assert with_(exp, ok, a4=32, a5=65) == -1                       # 2080 cells


def test_public_surface():
    from scanpaths_amd import inference
    from scanpaths_amd.utils import evaluation as E
    empty, KW = inspect.Parameter.empty, inspect.Parameter.KEYWORD_ONLY
    p = inspect.signature(M().recurrence_mask).parameters
    assert list(p) == ["map_shape", "frame_size", "radius"] and all(v.default is empty for v in p.values())
    p = inspect.signature(M().recurrence_counts).parameters
    assert list(p) == ["scanpaths", "groups", "n_groups", "frame_size", "map_shape", "max_steps", "radius", "min_line"]
    assert all(p[k].kind is KW for k in ("max_steps", "radius", "min_line")) and all(p[k].default is empty for k in p)
    p = inspect.signature(M().recurrence_expectation).parameters
    assert list(p) == ["probs", "row_groups", "n_groups", "min_length", "max_steps", "radius", "frame_size", "map_shape"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("min_length", "max_steps", "radius", "frame_size"))
    assert p["map_shape"].default is None
    assert list(inspect.signature(M().recurrence_measures).parameters) == ["rqa"]
    assert list(inspect.signature(M().recurrence_summary).parameters) == ["table"]
    assert list(inspect.signature(M().recurrence_comparison).parameters) == ["table", "human_table"]
    p = inspect.signature(E.recurrence_statistics_evaluation).parameters
    assert list(p) == ["gt_fix_vectors", "predict_fix_vectors", "gt_keys", "predict_keys", "frame_size", "map_shape", "max_steps", "radius",
                       "min_line", "groups", "image_keys"]
    assert all(p[k].kind is KW and p[k].default is empty for k in list(p)[4:9]) and p["groups"].default is None
    p = inspect.signature(E.recurrence_statistics_human_evaluation).parameters
    assert list(p) == ["gt_fix_vectors", "gt_keys", "frame_size", "map_shape", "max_steps", "radius", "min_line", "groups", "image_keys"]
    p = inspect.signature(E.recurrence_statistics_model_evaluation).parameters
    assert list(p) == ["predict", "keys", "min_length", "max_steps", "radius", "performances", "frame_size", "map_shape", "groups", "human_table"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("min_length", "max_steps", "radius"))
    assert list(inspect.signature(E.RecurrenceStatisticsTable.__init__).parameters) == ["self", "max_steps"]
    assert list(inspect.signature(E.RecurrenceStatisticsTable.result).parameters) == ["self", "human_table"]
    assert issubclass(E.RecurrenceStatisticsTable, E._StatisticsTable) and E._RECURRENCE == ("recurrence", "table", "points", "E")
    p = inspect.signature(inference.run_recurrence_statistics_loop).parameters
    assert list(p) == ["model", "loader", "min_length", "max_steps", "radius", "human_table", "ablate_attention_info", "frame_size", "map_shape"]
    assert all(p[k].kind is KW and p[k].default is empty for k in ("min_length", "max_steps", "radius"))
    # what the saccade and turn statistics call keeps its defaults
    from scanpaths_amd.utils.evaltools import _grouped
    p = inspect.signature(_grouped.grouped_counts).parameters
    assert p["library"].default is None and p["per_scanpath"].default is None
    assert inspect.signature(_grouped.grouped_expectation).parameters["library"].default is None


def test_refusals_come_before_any_device_call(monkeypatch):
    from scanpaths_amd import hip, inference
    from scanpaths_amd.utils import evaluation as E

    def no_lib():
        raise AssertionError("validation must come first")

    monkeypatch.setattr(M(), "_device", no_lib)
    monkeypatch.setattr(hip, "lib", no_lib)
    monkeypatch.setattr(hip, "stats_lib", no_lib)
    sp = np.array([[1.0, 1.0, 0.2], [5.0, 3.0, 0.3], [9.0, 3.0, 0.3]])
    frame, shape = (24, 40), (3, 5)
    counts = M().recurrence_counts
    ok = dict(max_steps=6, radius=8.0, min_line=2)
    for missing in ok:
        with pytest.raises(TypeError):
            counts([sp], [0], 1, frame, shape, **{k: v for k, v in ok.items() if k != missing})
    for bad in (0, -1, 1.5, True, None, 65):
        with pytest.raises(ValueError, match="max_steps"):
            counts([sp], [0], 1, frame, shape, **dict(ok, max_steps=bad))
    for bad in (-1.0, float("nan"), float("inf"), None, True, "8"):
        with pytest.raises(ValueError, match="radius"):
            counts([sp], [0], 1, frame, shape, **dict(ok, radius=bad))
    for bad in (1, 0, -2, 2.5, None, True):
        with pytest.raises(ValueError, match="min_line"):
            counts([sp], [0], 1, frame, shape, **dict(ok, min_line=bad))
    with pytest.raises(ValueError, match="kernel limit"):
        counts([np.zeros((M().MAX_FIXATIONS + 1, 2))], [0], 1, frame, shape, **ok)
    for bad in ((0, 5), (3,), (3, -5), (2.5, 4), None, (3, 5, 7)):
        with pytest.raises(ValueError, match="map_shape"):
            counts([sp], [0], 1, frame, bad, **ok)
    with pytest.raises(ValueError, match="kernel limit"):
        counts([sp], [0], 1, frame, (32, 65), **ok)                                         # 2080 cells
    for bad in ([1], [-1], [2]):
        with pytest.raises(ValueError, match="out of range"):
            counts([sp], bad, 1, frame, shape, **ok)
    with pytest.raises(ValueError, match="one group per scanpath"):
        counts([sp, sp], [0], 1, frame, shape, **ok)
    for bad in (0, -1, None, 1.5):
        with pytest.raises(ValueError, match="n_groups"):
            counts([sp], [0], bad, frame, shape, **ok)
    for bad in ((0, 32), (24, float("inf")), (float("nan"), 32)):
        with pytest.raises(ValueError, match="frame_size"):
            counts([sp], [0], 1, bad, shape, **ok)
    with pytest.raises(ValueError, match="scanpath is an"):
        counts([np.zeros((3, 1))], [0], 1, frame, shape, **ok)
    res = counts([], [], 2, frame, shape, max_steps=3, radius=0, min_line=2)                # nothing to count: zeros, no device
    assert res["counts"].dtype == np.int64 and res["counts"].shape == (2, 3, 3) and not res["counts"].any()
    assert res["points"].dtype == res["dropped"].dtype == res["rqa"].dtype == np.int32
    assert res["points"].shape == (0,) and res["rqa"].shape == (0, 6)
    for bad in (-0.5, float("nan"), None):
        with pytest.raises(ValueError, match="radius"):
            M().recurrence_mask(shape, frame, bad)

    T = 4
    probs = torch.full((2, T, 16), 1.0 / 16)
    exp = M().recurrence_expectation
    ok = dict(min_length=1, max_steps=4, radius=8.0, frame_size=frame, map_shape=shape)
    for missing in ("min_length", "max_steps", "radius", "frame_size"):
        with pytest.raises(TypeError):
            exp(probs, [0, 0], 1, **{k: v for k, v in ok.items() if k != missing})
    for bad in (-1, 1.5, True, None):
        with pytest.raises(ValueError, match="min_length"):
            exp(probs, [0, 0], 1, **dict(ok, min_length=bad))
    for bad in (0, 2.5, None, 65):
        with pytest.raises(ValueError, match="max_steps"):
            exp(probs, [0, 0], 1, **dict(ok, max_steps=bad))
    for bad in (-1, float("nan"), float("inf"), None):
        with pytest.raises(ValueError, match="radius"):
            exp(probs, [0, 0], 1, **dict(ok, radius=bad))
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
    for bad in (np.zeros((3, 4)), np.zeros(9), np.zeros((0, 0))):
        with pytest.raises(ValueError, match="recurrence table"):
            M().recurrence_summary(bad)
    with pytest.raises(ValueError, match="one shape"):
        M().recurrence_comparison(np.ones((5, 5)), np.ones((9, 9)))
    for bad in (np.zeros((2, 5)), np.zeros(5), -np.ones((1, 6))):
        with pytest.raises(ValueError, match="rqa"):
            M().recurrence_measures(bad)

    # the keyed layer
    ev = E.recurrence_statistics_evaluation
    kw = dict(frame_size=frame, map_shape=shape, max_steps=3, radius=8.0, min_line=2)
    for missing in kw:
        with pytest.raises(TypeError):
            ev([sp], [sp], ["a"], ["a"], **{k: v for k, v in kw.items() if k != missing})
    with pytest.raises(ValueError, match="max_steps"):
        ev([sp], [sp], ["a"], ["a"], **dict(kw, max_steps=65))
    with pytest.raises(ValueError, match="min_line"):
        ev([sp], [sp], ["a"], ["a"], **dict(kw, min_line=1))
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
    mv = E.recurrence_statistics_model_evaluation
    mkw = dict(min_length=1, max_steps=3, radius=8.0, frame_size=frame, map_shape=shape)
    for missing in ("min_length", "max_steps", "radius"):
        with pytest.raises(TypeError):
            mv(one, ["a", "b"], **{k: v for k, v in mkw.items() if k != missing})
    with pytest.raises(ValueError, match="predict lacks 'good_all_actions_prob'"):
        mv(one, ["a", "b"], performances=[[True], [False]], **mkw)
    with pytest.raises(ValueError, match="predict lacks 'all_actions_prob'"):
        mv(two, ["a", "b"], **mkw)
    with pytest.raises(ValueError, match="one list of performances per sample"):
        mv(two, ["a", "b"], performances=[[True]], **mkw)
    with pytest.raises(ValueError, match="map_shape"):
        mv(one, ["a", "b"], **dict(mkw, map_shape=None))
    with pytest.raises(ValueError, match="human_table"):
        mv(one, ["a", "b"], human_table=np.ones((9, 9)), **mkw)
    with pytest.raises(ValueError, match="has no group"):
        mv(one, ["a", "b"], groups={"a": 0}, **mkw)
    for bad in (0, 65):
        with pytest.raises(ValueError, match="max_steps"):
            E.RecurrenceStatisticsTable(bad)
        with pytest.raises(ValueError, match="max_steps"):
            inference.run_recurrence_statistics_loop(None, [], min_length=1, max_steps=bad, radius=8.0)


def test_no_cpu_path(monkeypatch):
    from scanpaths_amd import hip
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(hip.HipError, match="no CPU path"):
        M().recurrence_counts([np.array([[1.0, 1.0]])], [0], 1, (24, 32), (3, 4), max_steps=2, radius=8.0, min_line=2)
    with pytest.raises(hip.HipError, match="no CPU path"):
        M().recurrence_expectation(torch.zeros(1, 2, 13), [0], 1, min_length=0, max_steps=2, radius=8.0, frame_size=(24, 32), map_shape=(3, 4))


# ---- the mask ---------------------------------------------------------------------------------------------------------------------------
def test_mask_by_hand():
    # a 2 x 3 map on 20 x 45 pixels: cells of 15 (wide) x 10 (high); lattice rows dr = -1, 0, 1, columns dc = -2 .. 2
    m = M().recurrence_mask((2, 3), (20.0, 45.0), 16.0)
    assert m.dtype == np.uint8 and m.shape == (3, 5) and m.flags["C_CONTIGUOUS"]
    # (dr, dc) = (0, +-1): 15 px; (+-1, 0): 10 px; (+-1, +-1): sqrt(325) = 18.03 px; (0, +-2): 30 px
    assert m.tolist() == [[0, 0, 1, 0, 0], [0, 1, 1, 1, 0], [0, 0, 1, 0, 0]]
    assert M().recurrence_mask((2, 3), (20.0, 45.0), 15.0).tolist() == m.tolist()           # on the boundary: <=, in float64
    assert M().recurrence_mask((2, 3), (20.0, 45.0), np.nextafter(15.0, 0)).tolist() == [[0, 0, 1, 0, 0], [0, 0, 1, 0, 0], [0, 0, 1, 0, 0]]
    assert M().recurrence_mask((2, 3), (20.0, 45.0), 18.1).tolist() == [[0, 1, 1, 1, 0], [0, 1, 1, 1, 0], [0, 1, 1, 1, 0]]
    for shape, frame in (((2, 3), (20.0, 45.0)), ((1, 1), (75.0, 100.0)), ((5, 7), (100.0, 300.0)), ((30, 40), (240, 320))):
        Hm, Wm = shape
        zero = M().recurrence_mask(shape, frame, 0)                                         # only the same cell
        assert zero.sum() == 1 and zero[Hm - 1, Wm - 1] == 1
        assert M().recurrence_mask(shape, frame, float(np.hypot(*frame))).all()             # the frame's diagonal: all ones
        for radius in (0.0, 16.0, 47.5, 1e9):
            assert np.array_equal(M().recurrence_mask(shape, frame, radius), R.mask(shape, frame, radius)), (shape, radius)
        m = M().recurrence_mask(shape, frame, 33.0)
        assert np.array_equal(m, m[::-1, ::-1])                                             # d and -d are equally long


# ---- the restatement against exhaustive enumeration ------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_steps", ["below", "above"])
@pytest.mark.parametrize("min_length", ["0", "1", "T+1"])
@pytest.mark.parametrize("shape,T,radius", [((1, 1), 3, 0.0), ((2, 3), 4, 16.0), ((2, 2), 5, 40.0)])
def test_restatement_equals_the_exhaustive_enumeration(shape, T, radius, min_length, max_steps):
    """All (1 + P)^T action sequences under the sampler's rule (terminate masked for t < min_length, the first terminate ends the
    scanpath; only the first max_steps fixations count), weighted in exact rationals: every entry of the table -- recurrent pairs,
    pairs, fixations -- and "points".  The bound is relative: ((1 + P)^T + T) * 2^-53, the number of terms an enumeration adds into one
    entry plus the T factors of a term; all terms are non-negative.  (The restatement's own longest chain is far shorter: per step a
    sum of depth <= P, a division, a subtraction and a product, then a blur and a dot product of at most P terms each -- at most
    T (P + 3) + 2 P roundings, 9 for the one-cell case, whose sums add zeros only.)"""
    Hm, Wm = shape
    P = Hm * Wm
    min_length = {"0": 0, "1": 1, "T+1": T + 1}[min_length]
    K = T - 1 if max_steps == "below" else T + 2
    frame = (20.0, 45.0) if shape == (2, 3) else (75.0, 100.0)
    table = R.mask(shape, frame, radius)
    g = np.random.default_rng(13 * T + P)
    probs = g.uniform(0.05, 1.0, (1, T, 1 + P)).astype(np.float32)       # unnormalised on purpose
    exact = [[Fraction(float(v)) for v in probs[0, t]] for t in range(T)]
    step = []
    for t in range(T):
        allowed = range(1, 1 + P) if t < min_length else range(1 + P)
        total = sum(exact[t][k] for k in allowed)
        step.append([exact[t][a] / total if a in allowed else Fraction(0) for a in range(1 + P)])
    want = [[Fraction(0)] * K for _ in range(K)]
    mass = Fraction(0)
    for seq in itertools.product(range(1 + P), repeat=T):
        w = Fraction(1)
        for t, a in enumerate(seq):
            w *= step[t][a]
            if not w:
                break
        if not w:
            continue
        mass += w
        fix = list(itertools.takewhile(lambda a: a != 0, seq))[:K]       # the first terminate ends the scanpath
        cells = [((a - 1) // Wm, (a - 1) % Wm) for a in fix]
        for t, b in enumerate(cells):
            want[t][t] += w
            for s, a in enumerate(cells[:t]):
                want[t][s] += w
                if table[b[0] - a[0] + Hm - 1, b[1] - a[1] + Wm - 1]:
                    want[s][t] += w
    assert mass == 1
    wantf = np.array([[float(v) for v in row] for row in want])
    got = R.recurrence_expectation(probs, [0], 1, table, min_length, K)
    bound = ((1 + P) ** T + T) * 2.0 ** -53
    assert got["bad"].tolist() == [0] and got["E"].shape == (1, K, K)
    err = np.abs(got["E"][0] - wantf)
    print(shape, T, min_length, K, "worst relative error", float((err / np.maximum(wantf, 1e-300)).max()), "bound", bound)
    assert (err <= bound * wantf).all(), (got["E"][0], wantf)
    Tm = min(T, K)
    points = float(sum(want[s][t] for s in range(Tm) for t in range(s + 1, Tm)))
    assert abs(got["points"][0] - points) <= bound * points
    assert wantf[0, 0] == 1.0 if min_length > 0 else wantf[0, 0] < 1.0
    assert not wantf[Tm:].any() and not wantf[:, Tm:].any()              # beyond Tm the table stays empty
    if radius == 0.0 and P == 1:
        assert np.array_equal(np.triu(wantf, 1), np.tril(wantf, -1).T)   # one cell: every pair is recurrent


def test_expectation_restatement_rules_by_hand():
    # uniform maps, no terminate mass (min_length beyond T): every pair exists, and X = the share of cell pairs within the mask
    shape, P = (2, 3), 6
    table = R.mask(shape, (20.0, 45.0), 16.0)                            # the cell itself and its four neighbours
    within = sum(int(table[b // 3 - a // 3 + 1, b % 3 - a % 3 + 2]) for a in range(P) for b in range(P))
    assert within == 6 + 2 * 7                                           # 6 stays, 4 horizontal and 3 vertical neighbour pairs, both ways
    probs = np.full((3, 4, 1 + P), 0.5, dtype=np.float32)
    got = R.recurrence_expectation(probs, [0, 2, 0], 2, table, 5, 3)     # row 1: a group that does not exist; Tm = 3 of T = 4
    assert got["bad"].tolist() == [0, -1, 0] and np.isnan(got["points"][1]) and not got["E"][1].any()
    E = got["E"][0]
    assert np.array_equal(np.tril(E), 2.0 * np.tril(np.ones((3, 3))))    # two rows: every fixation and every pair exists
    assert np.allclose(np.triu(E, 1), 2.0 * within / 36.0 * np.triu(np.ones((3, 3)), 1), rtol=1e-14, atol=0)
    assert abs(got["points"][0] - 3 * within / 36.0) <= 1e-14
    assert R.recurrence_expectation(probs, [0, 0, 0], 1, table, 5, 1)["E"].tolist() == [[[3.0]]]        # Tm = 1: fixations only
    # terminate mass: p_0 = the cells' sum from min_length = 1 on, q = 1/2: fixation t is reached with (1/2)^t, pair (s, t) likewise
    half = np.concatenate([np.full((1, 4, 1), 3.0, np.float32), probs[:1, :, 1:]], 2)
    E = R.recurrence_expectation(half, [0], 1, table, 1, 64)["E"][0]
    assert E.shape == (64, 64) and not E[4:].any() and not E[:, 4:].any()
    assert np.diag(E)[:4].tolist() == [1.0, 0.5, 0.25, 0.125] and E[1, 0] == 0.5 and E[3, 0] == 0.125 and E[3, 2] == 0.125
    assert abs(E[0, 3] - 0.125 * within / 36.0) <= 1e-15
    # a bad row: a zero step, NaN, inf -- only where t < Tm
    for value in (0.0, float("nan"), float("inf")):
        broken = probs.copy()
        broken[1, 3, 1:] = value if value == 0.0 else broken[1, 3, 1:]
        broken[1, 3, 3] = value
        got = R.recurrence_expectation(broken, [0, 0, 1], 2, table, 5, 64)
        assert got["bad"].tolist() == [0, 1, 0] and np.isnan(got["points"][1]) and got["E"][0, 0, 0] == 1.0
        assert R.recurrence_expectation(broken, [0, 0, 1], 2, table, 5, 3)["bad"].tolist() == [0, 0, 0]        # t = 3 >= Tm: never read


# ---- RQA by hand --------------------------------------------------------------------------------------------------------------------------
def _path(cells):
    """fixations at the centres of the named cells of a 3 x 4 map on 30 x 40 pixels (cells of 10 x 10); None: a NaN fixation"""
    at = {"A": (5.0, 5.0), "B": (25.0, 5.0), "C": (5.0, 25.0), "D": (35.0, 25.0)}
    return np.array([at[c] if c is not None else (float("nan"), 1.0) for c in cells]).reshape(-1, 2)


def _rqa(cells, min_line, max_steps=64):
    table = R.mask((3, 4), (30.0, 40.0), 0.0)                            # radius 0: the same cell only
    res = R.recurrence_counts([_path(cells)], [0], 1, (30.0, 40.0), (3, 4), max_steps, table, min_line)
    got = M().recurrence_measures(res["rqa"])
    want = R.measures(res["rqa"][0])
    assert set(got) == set(want) == {"REC", "DET", "LAM", "CORM"}
    for k in got:
        assert got[k].dtype == np.float64 and got[k].shape == (1,)
        assert np.array_equal(got[k], [want[k]], equal_nan=True), (k, got[k], want[k])
    return res, {k: float(v[0]) for k, v in got.items()}


def test_rqa_integers_and_measures_by_hand():
    # A B C A B C: the points (0, 3), (1, 4), (2, 5) -- ONE diagonal line of three
    res, m = _rqa("ABCABC", 3)
    assert res["rqa"][0].tolist() == [6, 3, 3, 0, 0, 9] and res["points"].tolist() == [3]    # a line of exactly L
    assert m == {"REC": 100.0 * 6 / 30, "DET": 100.0, "LAM": 0.0, "CORM": 100.0 * 9 / 15}
    assert _rqa("ABCABC", 2)[0]["rqa"][0].tolist() == [6, 3, 3, 0, 0, 9]
    res, m = _rqa("ABCABC", 4)                                           # the same line is L - 1 long: not counted
    assert res["rqa"][0].tolist() == [6, 3, 0, 0, 0, 9] and m["DET"] == 0.0 and m["REC"] == 20.0
    want = np.zeros((6, 6), np.int64)
    want[np.tril_indices(6)] = 1                                         # every fixation, every pair
    want[0, 3] = want[1, 4] = want[2, 5] = 1
    assert np.array_equal(res["counts"][0, :6, :6], want) and res["counts"].sum() == want.sum()
    # a dropped fixation inside the line: it is in no pair and breaks the line in original ordinals (no compaction)
    res, m = _rqa(["A", "B", "C", "A", None, "C"], 2)
    assert res["rqa"][0].tolist() == [5, 2, 0, 0, 0, 6] and res["dropped"].tolist() == [1]
    assert m == {"REC": 100.0 * 4 / 20, "DET": 0.0, "LAM": 0.0, "CORM": 100.0 * 6 / (4 * 2)}
    assert not res["counts"][0, 4].any() and not res["counts"][0, :, 4].any()
    # A A A B: (0, 1), (0, 2), (1, 2): a horizontal pair in row 0, a vertical pair in column 2 and a diagonal pair
    res, m = _rqa("AAAB", 2)
    assert res["rqa"][0].tolist() == [4, 3, 2, 2, 2, 4]
    assert m == {"REC": 100.0 * 6 / 12, "DET": 100.0 * 2 / 3, "LAM": 100.0 * 4 / 6, "CORM": 100.0 * 4 / 9}
    assert _rqa("AAAB", 3)[0]["rqa"][0].tolist() == [4, 3, 0, 0, 0, 4]
    # A A A A A: row i holds 4 - i consecutive points, column j holds j, the diagonal of lag l holds 5 - l
    assert _rqa("AAAAA", 3)[0]["rqa"][0].tolist() == [5, 10, 4 + 3, 4 + 3, 3 + 4, 1 * 4 + 2 * 3 + 3 * 2 + 4]
    assert _rqa("AAAAA", 3, max_steps=3)[0]["rqa"][0].tolist() == [3, 3, 0, 0, 0, 4]         # only the first three fixations
    # N < 2 and R = 0
    res, m = _rqa("A", 2)
    assert res["rqa"][0].tolist() == [1, 0, 0, 0, 0, 0] and all(np.isnan(v) for v in m.values())
    res, m = _rqa("", 2)
    assert res["rqa"][0].tolist() == [0] * 6 and all(np.isnan(v) for v in m.values())
    res, m = _rqa("ABCD", 2)
    assert res["rqa"][0].tolist() == [4, 0, 0, 0, 0, 0] and m["REC"] == 0.0 and all(np.isnan(m[k]) for k in ("DET", "LAM", "CORM"))
    res, m = _rqa([None, "A", None], 2)
    assert res["rqa"][0].tolist() == [1, 0, 0, 0, 0, 0] and np.isnan(m["REC"])
    assert R.recurrence_counts([np.zeros((65, 2))], [0], 1, (30.0, 40.0), (3, 4), 5, R.mask((3, 4), (30.0, 40.0), 0.0), 2)["rqa"].tolist() \
        == [[-1] * 6]
    many = M().recurrence_measures(np.array([[6, 3, 3, 0, 0, 9], [1, 0, 0, 0, 0, 0]]))
    assert many["REC"][0] == 20.0 and np.isnan(many["REC"][1]) and M().recurrence_measures([6, 3, 3, 0, 0, 9])["DET"].tolist() == [100.0]


# ---- the host statistics by hand ----------------------------------------------------------------------------------------------------------
def _both(table):
    got, want = M().recurrence_summary(table), R.summary(table)
    assert set(got) == {"fixations", "pairs", "points", "REC", "recurrence_by_lag", "mean_lag", "mean_lag_chance"} == set(want)
    for k in got:                   # sums of at most 64^2 / 2 non-negative terms in two orders
        assert np.allclose(np.asarray(got[k], dtype=np.float64), np.asarray(want[k], dtype=np.float64), rtol=1e-12, atol=0, equal_nan=True), k
    return got


def test_summary_and_comparison_by_hand():
    t = np.array([[4, 1, 2, 0], [4, 4, 0, 1], [3, 3, 3, 1], [2, 2, 2, 2]])
    s = _both(t)
    assert s["fixations"] == 13.0 and s["pairs"] == 16.0 and s["points"] == 5.0 and s["REC"] == 100.0 * 5 / 16
    assert s["recurrence_by_lag"].tolist() == [2.0 / 9.0, 3.0 / 5.0, 0.0] and s["recurrence_by_lag"].dtype == np.float64
    assert s["mean_lag"] == (1 * 2 + 2 * 3 + 3 * 0) / 5.0 and s["mean_lag_chance"] == (1 * 9 + 2 * 5 + 3 * 2) / 16.0
    s = _both(np.array([[3.0]]))                                         # one step: fixations only
    assert s["fixations"] == 3.0 and s["pairs"] == 0.0 and np.isnan(s["REC"]) and s["recurrence_by_lag"].shape == (0,)
    assert np.isnan(s["mean_lag"]) and np.isnan(s["mean_lag_chance"])
    t = np.zeros((4, 4))
    t[1, 0], t[2, 1], t[0, 0] = 2.0, 1.0, 3.0                            # pairs of lag 1 only, none recurrent
    s = _both(t)
    assert s["REC"] == 0.0 and np.isnan(s["mean_lag"]) and s["mean_lag_chance"] == 1.0
    assert s["recurrence_by_lag"][0] == 0.0 and np.isnan(s["recurrence_by_lag"][1:]).all()
    s = _both(np.zeros((5, 5)))
    assert np.isnan(s["REC"]) and np.isnan(s["recurrence_by_lag"]).all() and s["recurrence_by_lag"].shape == (4,)
    g = np.random.default_rng(3)
    _both(g.integers(0, 9, (9, 9)))
    _both(g.uniform(0, 1, (64, 64)))
    # the comparison
    a = np.array([[4, 1, 2, 0], [4, 4, 0, 1], [3, 3, 3, 1], [2, 2, 2, 2]])
    assert M().recurrence_comparison(a, 3 * a) == {"REC_difference": 0.0, "L1_by_lag": 0.0, "JSD_lag": 0.0}
    b = np.array([[4, 0, 0, 2], [4, 4, 0, 0], [4, 4, 4, 0], [4, 4, 4, 4]])                 # all recurrence at lag 3; a has none there
    c = M().recurrence_comparison(a, b)
    assert c["REC_difference"] == 100.0 * 5 / 16 - 100.0 * 2 / 24 and c["JSD_lag"] == 1.0
    assert abs(c["L1_by_lag"] - (2.0 / 9.0 + 3.0 / 5.0 + 2.0 / 4.0) / 3.0) <= 1e-16
    b[3, 0] = 0                                                          # no pair of lag 3 on the human side: that lag is left out
    assert abs(M().recurrence_comparison(a, b)["L1_by_lag"] - (2.0 / 9.0 + 3.0 / 5.0) / 2.0) <= 1e-16
    none = M().recurrence_comparison(a, np.zeros((4, 4)))
    assert np.isnan(none["REC_difference"]) and np.isnan(none["L1_by_lag"]) and np.isnan(none["JSD_lag"])
    x, y = g.uniform(0, 1, (9, 9)), g.integers(1, 4, (9, 9))
    c = M().recurrence_comparison(x, y)
    up = lambda t: [float(np.trace(t, offset=k)) for k in range(1, 9)]                      # noqa: E731
    from saccade_statistics_ref import jensen_shannon
    assert abs(c["JSD_lag"] - jensen_shannon(up(x), up(y))) <= 1e-15
    assert abs(c["REC_difference"] - (R.summary(x)["REC"] - R.summary(y)["REC"])) <= 1e-12


def test_table_merges_sums_and_derives_from_the_summed_tables():
    from scanpaths_amd.utils import evaluation as E
    g = np.random.default_rng(9)
    parts = [{"table_sum": g.integers(0, 5, (5, 5)), "human_table_sum": g.integers(1, 5, (5, 5)), "points_sum": 3, "scanpaths_count": 2,
              "fixations_dropped": 1, "rows_bad": 1, "summary": "not merged", "JSD_lag": 0.3,
              "by_group": {"t": {"table_sum": g.integers(0, 5, (5, 5)), "points_sum": 1}}} for _ in range(3)]
    table = E.RecurrenceStatisticsTable(5)
    for p in parts:
        table.add(p)
    out = table.result()
    tab, hum = sum(p["table_sum"] for p in parts), sum(p["human_table_sum"] for p in parts)
    assert np.array_equal(out["table_sum"], tab) and out["table_sum"].dtype == np.int64 and out["points_sum"] == 9      # integers: exact
    assert out["scanpaths_count"] == 6 and out["fixations_dropped"] == 3 and out["rows_bad"] == 3
    assert out["summary"]["points"] == float(np.triu(tab, 1).sum()) and out["human_summary"]["pairs"] == float(np.tril(hum, -1).sum())
    assert all(out[k] == v for k, v in M().recurrence_comparison(tab, hum).items())
    assert np.array_equal(out["by_group"]["t"]["table_sum"], sum(p["by_group"]["t"]["table_sum"] for p in parts))
    assert "JSD_lag" not in out["by_group"]["t"] and out["by_group"]["t"]["summary"]["fixations"] > 0
    other = g.uniform(0.1, 1, (5, 5))
    no_human = E.RecurrenceStatisticsTable(5)
    no_human.add({"table_sum": parts[0]["table_sum"]})
    assert "JSD_lag" not in no_human.result()
    assert no_human.result(other)["JSD_lag"] == M().recurrence_comparison(parts[0]["table_sum"], other)["JSD_lag"]
    assert parts[0]["table_sum"] is not no_human.parts["table_sum"]                          # add copies: the caller's array stays
    with pytest.raises(ValueError, match="the table's lattice"):
        no_human.add({"table_sum": np.zeros((9, 9))})
    # expectations: two halves merged equal one sum over the union within 4 * 2^-53 relative per added table -- every term is
    # non-negative, and each side is within (tables - 1) * 2^-53 of the true sum
    rows = [g.uniform(0, 1, (5, 5)) for _ in range(4)]
    halves = E.RecurrenceStatisticsTable(5)
    halves.add({"table_sum": rows[0] + rows[1], "points_sum": float((rows[0] + rows[1]).sum()), "rows_count": 2})
    halves.add({"table_sum": rows[2] + rows[3], "points_sum": float((rows[2] + rows[3]).sum()), "rows_count": 2})
    union = ((rows[0] + rows[1]) + rows[2]) + rows[3]
    merged = halves.result()
    assert merged["rows_count"] == 4 and np.allclose(merged["table_sum"], union, rtol=4 * 2.0 ** -53 * 2, atol=0)
    assert abs(merged["points_sum"] - union.sum()) <= 1e-13 * union.sum()
