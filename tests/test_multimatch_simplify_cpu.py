"""CPU-only checks of MultiMatch's scanpath simplification: the host restatement simplify_scanpath on cases worked out
by hand (halving of a collinear walk, the amplitude pass on a staircase, the even-offset rule within runs of candidates, the last
fixation, zero-length saccades), its properties over seeded random scanpaths, docomparison(grouping=True) and its scoring rule, every
argument refusal of the Python layer (raised before a device or the library is touched) and the two new C entry points."""
import os

import numpy as np
import pytest

import abi
import multimatch_simplify_cases as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FV = {"names": ("start_x", "start_y", "duration"), "formats": ("f8", "f8", "f8")}


def _records(a):
    r = np.zeros(len(a), dtype=FV)
    r["start_x"], r["start_y"], r["duration"] = a[:, 0], a[:, 1], a[:, 2]
    return r


@pytest.mark.parametrize("name", sorted(C.CONSTRUCTED))
def test_constructed_cases(name):
    from scanpaths_amd.utils.evaltools.multimatch import simplify_scanpath
    path, thresholds, keep = C.CONSTRUCTED[name]
    got = simplify_scanpath(path, *thresholds)
    assert got.dtype == np.float64 and np.array_equal(got, path[keep]), (name, got)
    assert np.array_equal(simplify_scanpath(_records(path), *thresholds), got)           # fixation records are taken too


def test_collinear_walk_halves_round_by_round(monkeypatch):
    """33 fixations: 32 -> 16 -> 8 -> 4 -> 2 -> 1 saccades = 5 rounds that delete something; 64 fixations: 63 -> 32 first = 6.  (A
    sixth / seventh round would find nothing; the host loop does not run it on a path that is down to 2 fixations.)"""
    from scanpaths_amd.utils.evaltools import multimatch as M
    for n, rounds in ((33, 5), (64, 6)):
        calls = []
        real = M._simplify_pass
        monkeypatch.setattr(M, "_simplify_pass", lambda rows, kind, *a: calls.append(kind) or real(rows, kind, *a))
        got = M.simplify_scanpath(C.walk(n), 45.0, 0.3, 0.0)
        monkeypatch.setattr(M, "_simplify_pass", real)
        assert np.array_equal(got, C.walk(n)[[0, n - 1]])
        assert calls.count("direction") == calls.count("amplitude") == rounds, (n, calls)


def test_thresholds_zero_are_the_identity_and_leave_the_scores_alone():
    from scanpaths_amd.utils.evaltools.multimatch import docomparison, simplify_scanpath
    lattice, uniform = C.random_paths(11, 20)
    for p in lattice + uniform:
        assert np.array_equal(simplify_scanpath(p, 0, 0, 0), p)
        assert np.array_equal(simplify_scanpath(p, 0.0, 0.3, 0.0), p)                  # no direction pass, no amplitude candidates
        assert np.array_equal(simplify_scanpath(p, 45.0, 0.0, 40.0), p)                # no duration is below 0
    short = [p for p in lattice + uniform if len(p) <= 24]
    assert len(short) >= 6
    for a, b in zip(short[::2], short[1::2]):
        with np.errstate(all="ignore"):
            plain = docomparison(_records(a), _records(b), screensize=[320, 240])
            grouped = docomparison(_records(a), _records(b), screensize=[320, 240], grouping=True, TDir=0.0, TDur=0.0, TAmp=0.0)
        assert np.array_equal(np.array(plain), np.array(grouped), equal_nan=True)


def test_properties_over_random_scanpaths():
    """idempotent; first and last row kept; a subsequence of the input rows; not vacuous: at least half of the scanpaths of 3 or
    more fixations get shorter at (45 degrees, 0.3, 40 px), on the lattice and off it"""
    from scanpaths_amd.utils.evaltools.multimatch import simplify_scanpath
    for kind, paths in zip(("lattice", "uniform"), C.random_paths(7, 1000)):
        shorter = eligible = 0
        for p in paths:
            s = simplify_scanpath(p, *C.THRESHOLDS)
            assert np.array_equal(simplify_scanpath(s, *C.THRESHOLDS), s)
            assert 1 <= len(s) <= len(p) and np.array_equal(s[0], p[0]) and np.array_equal(s[-1], p[-1])
            if len(p) < 3:
                assert np.array_equal(s, p)
                continue
            assert len(s) >= 2
            k = 0
            for row in s:                                                  # rows of s appear in p in order
                while not np.array_equal(p[k], row):
                    k += 1
                k += 1
            eligible += 1
            shorter += len(s) < len(p)
        print(f"{kind}: {shorter} of {eligible} scanpaths of 3 or more fixations got shorter")
        assert eligible > 900 and 2 * shorter >= eligible, (kind, shorter, eligible)


def test_scoring_rule_looks_at_the_original_lengths():
    from scanpaths_amd.utils.evaltools.multimatch import docomparison, simplify_scanpath
    three, other = C.walk(3), C.staircase(6)
    assert len(simplify_scanpath(three, 45.0, 0.3, 0.0)) == 2
    got = docomparison(_records(three), _records(other), screensize=[320, 240], grouping=True, TDir=45.0, TDur=0.3, TAmp=0.0)
    assert len(got) == 5 and np.isfinite(got).all(), got
    got = docomparison(_records(other), _records(three), screensize=[320, 240], grouping=True, TDir=45.0, TDur=0.3, TAmp=0.0)
    assert np.isfinite(got).all(), got
    both = docomparison(_records(three), _records(three), screensize=[320, 240], grouping=True, TDir=45.0, TDur=0.3, TAmp=0.0)
    assert both == [1.0] * 5                                               # one saccade against itself
    for a, b in ((C.walk(2), other), (other, C.walk(2)), (C.walk(1), C.walk(0))):
        got = docomparison(_records(a), _records(b), screensize=[320, 240], grouping=True, TDir=45.0, TDur=0.3, TAmp=40.0)
        assert len(got) == 5 and np.isnan(got).all()
    # the simplified paths are what is scored: equal to the plain score of the host-simplified paths
    a, b = C.random_paths(5, 4, lengths=[9, 14])[0][:2]
    sa, sb = simplify_scanpath(a, *C.THRESHOLDS), simplify_scanpath(b, *C.THRESHOLDS)
    assert len(sa) >= 3 and len(sb) >= 3
    with np.errstate(all="ignore"):
        assert docomparison(_records(a), _records(b), [320, 240], True, *C.THRESHOLDS) == docomparison(_records(sa), _records(sb), [320, 240])


BAD = [(-1.0, 0.3, 40.0), (180.5, 0.3, 40.0), (float("nan"), 0.3, 40.0), (float("inf"), 0.3, 40.0), (45.0, -0.1, 40.0),
       (45.0, float("nan"), 40.0), (45.0, float("inf"), 40.0), (45.0, 0.3, -1.0), (45.0, 0.3, float("nan")), (45.0, 0.3, float("inf")),
       (None, 0.3, 40.0)]


@pytest.mark.parametrize("bad", BAD)
def test_bad_thresholds_are_refused_before_any_device_work(bad):
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import multimatch as M
    p = [_records(C.walk(5)), _records(C.staircase(5))]
    tdir, tdur, tamp = bad
    with pytest.raises(ValueError):
        M.simplify_scanpath(p[0], tdir, tdur, tamp)
    with pytest.raises(ValueError):
        M.docomparison(p[0], p[1], [320, 240], grouping=True, TDir=tdir, TDur=tdur, TAmp=tamp)
    with pytest.raises(ValueError):
        M.simplify_scanpaths(p, TDir=tdir, TDur=tdur, TAmp=tamp)
    with pytest.raises(ValueError):
        M.multimatch_pairs(p, [(0, 1)], [320, 240], grouping=True, TDir=tdir, TDur=tdur, TAmp=tamp)
    with pytest.raises(ValueError):
        E.evaluation_performance_related([[p[0]]], [p[1]], [[True]], [True], multimatch_grouping=bad)
    with pytest.raises(ValueError):
        E.evaluation([[p[0]]], [p[1]], multimatch_grouping=bad)
    with pytest.raises(ValueError):
        E.human_evaluation([], multimatch_grouping=bad)
    with pytest.raises(ValueError):
        E.human_evaluation_free_viewing([], multimatch_grouping=bad)


def test_other_refusals_and_empty_calls_touch_no_device():
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import multimatch as M
    p = [C.walk(5), C.walk(65)]
    with pytest.raises(ValueError, match="64"):
        M.simplify_scanpaths(p, TDir=45.0, TDur=0.3, TAmp=40.0)
    with pytest.raises(ValueError, match="64"):
        M.multimatch_pairs([_records(a) for a in p], [(0, 1)], [320, 240], grouping=True, TDir=45.0, TDur=0.3, TAmp=40.0)
    with pytest.raises(ValueError, match="columns"):
        M.simplify_scanpaths([np.zeros((4, 2))], TDir=45.0, TDur=0.3, TAmp=40.0)
    with pytest.raises(ValueError, match="columns"):
        M.simplify_scanpaths([np.zeros((4, 3)), np.zeros((4, 5))], TDir=45.0, TDur=0.3, TAmp=40.0)
    for bad in ([(0, 2)], [(-1, 0)]):
        with pytest.raises(ValueError, match="out of range"):
            M.multimatch_pairs([_records(C.walk(5))] * 2, bad, [320, 240], grouping=True, TDir=45.0, TDur=0.3, TAmp=40.0)
    with pytest.raises(ValueError, match="triple"):
        E.evaluation([[_records(p[0])]], [_records(p[0])], multimatch_grouping=(45.0, 0.3))
    assert M.simplify_scanpaths([], TDir=45.0, TDur=0.3, TAmp=40.0) == []
    got = M.multimatch_pairs([_records(C.walk(5))], [], [320, 240], grouping=True, TDir=45.0, TDur=0.3, TAmp=40.0)
    assert got.shape == (0, 5)


def test_a_callable_gets_the_package_signature():
    """a user-supplied MultiMatch (or the installed package) is called with grouping=True, TDir=, TDur=, TAmp="""
    from scanpaths_amd.utils.evaluation import _grouping_kwargs, _multimatch_rows
    seen = []

    def mm(a, b, screensize, **kw):
        seen.append((screensize, kw))
        return [0.5] * 5
    rows = _multimatch_rows(mm, [(C.walk(4), C.walk(5))], _grouping_kwargs((45, 0.3, 40)))
    assert rows == [[0.5] * 5] and seen == [([320, 240], {"grouping": True, "TDir": 45.0, "TDur": 0.3, "TAmp": 40.0})]
    _multimatch_rows(mm, [(C.walk(4), C.walk(5))], _grouping_kwargs(None))
    assert seen[1] == ([320, 240], {})


def test_new_entry_points_are_declared_bound_and_exported():
    from scanpaths_amd.utils.evaltools import multimatch as M
    lib = abi.assert_declared(C.NEW)
    assert lib.sp_scan_max_fixations() == M.MAX_FIXATIONS == 64
    src = open(os.path.join(ROOT, "scanpaths_amd", "utils", "evaltools", "multimatch.py")).read()
    assert "NotImplementedError" not in src


def test_launchers_refuse_bad_arguments_without_a_device():
    C.check_refusals(abi.raw_lib())
