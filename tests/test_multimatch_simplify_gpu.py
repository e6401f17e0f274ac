"""MultiMatch's scanpath simplification on the device (csrc/scansimplify.hip, one wavefront per scanpath) against the
host restatement utils/evaltools/multimatch.simplify_scanpath, its checker.  The kernel only copies rows, so the comparison is bit for
bit: any difference is a wrong decision.  Then the grouped pair scorer (sp_scan_simplify + sp_scan_multimatch_gated) against
docomparison(grouping=True) at the bars of test_dataset_eval_gpu.test_multimatch_on_the_device_matches_the_host_restatement, the
gated kernel against the plain one, and the keyed evaluation with multimatch_grouping."""
import numpy as np
import pytest
import torch

import abi
import multimatch_simplify_cases as C

pytestmark = pytest.mark.gpu
FV = {"names": ("start_x", "start_y", "duration"), "formats": ("f8", "f8", "f8")}
LENGTHS = [0, 1, 2, 3, 4, 5, 31, 32, 33, 63, 64]
TRIPLES = [(45.0, 0.3, 40.0), (0.0, 0.3, 40.0), (45.0, 0.3, 0.0), (180.0, 1e9, 1e9), (0.0, 0.0, 0.0)]


def _records(a):
    r = np.zeros(len(a), dtype=FV)
    r["start_x"], r["start_y"], r["duration"] = a[:, 0], a[:, 1], a[:, 2]
    return r


@pytest.fixture(scope="module")
def paths():
    """every length of LENGTHS 12 times on the lattice and 12 times off it, the 64-fixation collinear walk (the most rounds) and the
    constructed cases"""
    lattice, uniform = C.random_paths(19, 12 * len(LENGTHS), lengths=LENGTHS)
    return lattice + uniform + [C.walk(64), C.walk(33), C.staircase(64)] + [p for p, _, _ in C.CONSTRUCTED.values()]


@pytest.mark.parametrize("triple", TRIPLES)
def test_simplify_on_the_device_equals_the_host_restatement_bit_for_bit(paths, triple):
    from scanpaths_amd.utils.evaltools.multimatch import simplify_scanpath, simplify_scanpaths
    ref = [simplify_scanpath(p, *triple) for p in paths]
    got = simplify_scanpaths(paths, TDir=triple[0], TDur=triple[1], TAmp=triple[2])
    wide = [np.concatenate([p, np.full((len(p), 2), np.nan)], 1) for p in paths]          # ncol 5: columns 3, 4 must not be read
    got5 = simplify_scanpaths(wide, TDir=triple[0], TDur=triple[1], TAmp=triple[2])
    assert len(got) == len(got5) == len(paths)
    for k, (p, r, g, g5) in enumerate(zip(paths, ref, got, got5)):
        assert g.dtype == np.float64 and g.shape == r.shape and np.array_equal(g, r), (k, len(p), triple, r, g)
        assert np.array_equal(g5, r), (k, len(p), triple)
    eligible = [k for k, p in enumerate(paths) if len(p) >= 3]
    shorter = sum(len(ref[k]) < len(paths[k]) for k in eligible)
    print(f"{triple}: {shorter} of {len(eligible)} scanpaths of 3 or more fixations got shorter")
    if triple == TRIPLES[0]:
        assert 2 * shorter >= len(eligible), (shorter, len(eligible))
    if triple == TRIPLES[3]:
        assert all(len(ref[k]) == 2 for k in eligible[:40])
    if triple == TRIPLES[4]:
        assert shorter == 0


def test_constructed_cases_on_the_device():
    from scanpaths_amd.utils.evaltools.multimatch import simplify_scanpaths
    for name, (path, triple, keep) in C.CONSTRUCTED.items():
        got = simplify_scanpaths([path, path[:2], path], TDir=triple[0], TDur=triple[1], TAmp=triple[2])
        assert np.array_equal(got[0], path[keep]) and np.array_equal(got[2], path[keep]) and np.array_equal(got[1], path[:2]), name


def test_a_count_beyond_the_limit_writes_count_zero_and_nothing_else():
    """the kernel's own guard (the Python layer refuses such a scanpath earlier): counts 65 and -1 give count_out 0 and none of
    their rows is written"""
    from scanpaths_amd import hip
    L = hip.lib()
    fix = torch.from_numpy(C.walk(80)).cuda()
    start = torch.tensor([0, 5, 5, 3], dtype=torch.int64).cuda()
    count = torch.tensor([3, 65, -1, 2], dtype=torch.int32).cuda()
    out = torch.full((80, 3), -7.0, dtype=torch.float64).cuda()
    kept = torch.full((4,), -7, dtype=torch.int32).cuda()
    hip.check(L.sp_scan_simplify(hip.ptr(fix), 3, hip.ptr(start), hip.ptr(count), 4, 0.5, 0.3, 0.0, hip.ptr(out), hip.ptr(kept),
                                 hip.stream()), "sp_scan_simplify")
    assert kept.cpu().tolist() == [2, 0, 0, 2]
    o = out.cpu().numpy()
    assert np.array_equal(o[:2], C.walk(80)[[0, 2]]) and np.array_equal(o[3:5], C.walk(80)[3:5])
    assert (o[2] == -7.0).all() and (o[5:] == -7.0).all()


@pytest.fixture(scope="module")
def scored():
    """60 scanpaths of 1 .. 24 fixations (half on the lattice), the gate cases, about 400 seeded pairs: host reference once"""
    from scanpaths_amd.utils.evaltools.multimatch import docomparison, simplify_scanpath
    rng = np.random.Generator(np.random.PCG64(31))
    paths = [(C.lattice_path if k % 2 else C.uniform_path)(rng, int(rng.integers(1, 25))) for k in range(60)]
    paths += [C.walk(3), C.walk(2), C.staircase(6), C.walk(24)]            # 60: simplifies to 2 fixations; 61: too short; 62; 63
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, 60, (400, 2))] + [(60, 62), (62, 60), (60, 60), (61, 62), (62, 61), (63, 60)]
    recs = [_records(p) for p in paths]
    with np.errstate(all="ignore"):
        ref = np.array([docomparison(recs[a], recs[b], screensize=[320, 240], grouping=True, TDir=45.0, TDur=0.3, TAmp=40.0)
                        for a, b in pairs], dtype=np.float64)
    kept = [len(simplify_scanpath(p, *C.THRESHOLDS)) for p in paths]
    return paths, recs, pairs, ref, kept


def test_grouped_multimatch_on_the_device_matches_the_host_restatement(scored):
    from scanpaths_amd.utils.evaltools.multimatch import multimatch_pairs
    paths, recs, pairs, ref, kept = scored
    got = multimatch_pairs(recs, pairs, [320, 240], grouping=True, TDir=45.0, TDur=0.3, TAmp=40.0)
    assert got.shape == ref.shape == (len(pairs), 5)
    assert np.array_equal(np.isnan(ref), np.isnan(got)), np.argwhere(np.isnan(ref) != np.isnan(got))
    nan = np.isnan(ref).any(1)
    assert np.array_equal(nan, np.array([len(paths[a]) < 3 or len(paths[b]) < 3 for a, b in pairs]))
    worst = np.abs(ref[~nan] - got[~nan]).max(0)
    shorter = sum(kept[a] < len(paths[a]) or kept[b] < len(paths[b]) for (a, b), bad in zip(pairs, nan) if not bad)
    single = sum(kept[a] == 2 or kept[b] == 2 for (a, b), bad in zip(pairs, nan) if not bad)
    print(f"grouped MultiMatch device vs host over {len(pairs)} pairs ({int(nan.sum())} unscorable, {shorter} with a shorter path, "
          f"{single} with a one-saccade path): worst |diff| per value {worst}")
    assert nan.sum() > 10 and shorter > 10 and single >= 3
    assert (worst[[0, 2, 3, 4]] <= 1e-13).all() and worst[1] <= 1e-12, worst
    assert np.isfinite(got[400]).all() and np.isfinite(got[401]).all() and np.isnan(got[403]).all() and np.isnan(got[404]).all()


def test_zero_thresholds_and_equal_gate_change_nothing(scored):
    """grouping with (0, 0, 0) is the ungrouped call; sp_scan_multimatch_gated with gate_count = count is sp_scan_multimatch, in
    every bit"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools.multimatch import multimatch_pairs
    paths, recs, pairs, _, _ = scored
    plain = multimatch_pairs(recs, pairs, [320, 240])
    assert np.isnan(plain).any() and np.isfinite(plain).any()
    assert np.array_equal(multimatch_pairs(recs, pairs, [320, 240], grouping=True, TDir=0.0, TDur=0.0, TAmp=0.0), plain, equal_nan=True)
    assert np.array_equal(multimatch_pairs(recs, pairs, [320, 240], grouping=False, TDir=45.0, TDur=0.3, TAmp=40.0), plain, equal_nan=True)
    L = hip.lib()
    counts = np.array([len(p) for p in paths], dtype=np.int32)
    fix = torch.from_numpy(np.concatenate(paths, 0)).cuda()
    start = torch.from_numpy(np.cumsum(counts, dtype=np.int64) - counts).cuda()
    count = torch.from_numpy(counts).cuda()
    prd = torch.tensor(pairs, dtype=torch.int32).cuda()
    out = torch.zeros((2, len(pairs), 5), dtype=torch.float64).cuda()
    hip.check(L.sp_scan_multimatch(hip.ptr(fix), 3, hip.ptr(start), hip.ptr(count), hip.ptr(prd), len(pairs), 320.0, 240.0,
                                   hip.ptr(out[0]), hip.stream()), "sp_scan_multimatch")
    hip.check(L.sp_scan_multimatch_gated(hip.ptr(fix), 3, hip.ptr(start), hip.ptr(count), hip.ptr(count), hip.ptr(prd), len(pairs),
                                         320.0, 240.0, hip.ptr(out[1]), hip.stream()), "sp_scan_multimatch_gated")
    o = out.cpu().numpy()
    assert np.array_equal(o[0].view(np.int64), o[1].view(np.int64)) and np.array_equal(o[0], plain, equal_nan=True)


def test_c_entry_points_refuse_bad_arguments():
    C.check_refusals(abi.raw_lib())


def _fv(rng, n, k):
    return _records((C.lattice_path if k % 2 else C.uniform_path)(rng, n))


def _same(a, b):
    a, b = float(a), float(b)
    return a == b or (a != a and b != b)


def test_keyed_evaluation_with_grouping():
    """evaluation_performance_related and evaluation with multimatch_grouping: the device default against the host callable (means
    within 1e-6, per-image scores within 1e-9, as the ungrouped comparison), and None against a call without the keyword"""
    from scanpaths_amd.utils.evaltools.multimatch import docomparison
    from scanpaths_amd.utils.evaluation import evaluation, evaluation_performance_related
    rng = np.random.Generator(np.random.PCG64(44))
    n_img, g = 6, (45.0, 0.3, 40.0)
    gt = [[_fv(rng, int(rng.integers(2, 12)), k + j) for j in range(int(rng.integers(2, 6)))] for k in range(n_img)]
    perf = [[bool(rng.random() < 0.5) for _ in x] for x in gt]
    perf[0], perf[1] = [True] * len(perf[0]), [False] * len(perf[1])
    pred = [_fv(rng, int(rng.integers(3, 14)), k) for k in range(n_img)]
    alloc = [True, False, True, True, False, True]
    dev_out = evaluation_performance_related(gt, pred, perf, alloc, multimatch_grouping=g)
    with np.errstate(all="ignore"):
        host_out = evaluation_performance_related(gt, pred, perf, alloc, multimatch=docomparison, multimatch_grouping=g)
    plain = evaluation_performance_related(gt, pred, perf, alloc)
    none = evaluation_performance_related(gt, pred, perf, alloc, multimatch_grouping=None)
    for part in (0, 1):
        for cat in ("all", "right_answer", "wrong_answer"):
            for grp in ("MultiMatch", "ScanMatch", "VAME"):
                for key, v in host_out[part][cat][grp].items():
                    assert abs(float(dev_out[part][cat][grp][key]) - float(v)) <= 1e-6, (part, cat, grp, key)
                    assert _same(none[part][cat][grp][key], plain[part][cat][grp][key])
    for a, b in zip(dev_out[2], host_out[2]):
        assert np.allclose(a, b, rtol=0, atol=1e-9)
    assert all(np.array_equal(a, b) for a, b in zip(none[2], plain[2]))
    moved = max(abs(float(dev_out[0]["all"]["MultiMatch"][k]) - float(plain[0]["all"]["MultiMatch"][k])) for k in ("vector", "length"))
    assert moved > 1e-6, "the simplification left every score where it was: the case checks nothing"

    gt2 = [[_fv(rng, int(rng.integers(3, 12)), k + j) for j in range(3)] for k in range(4)]
    pred2 = [_fv(rng, int(rng.integers(3, 14)), k) for k in range(4)]
    dev2 = evaluation(gt2, pred2, multimatch_grouping=g)
    with np.errstate(all="ignore"):
        host2 = evaluation(gt2, pred2, multimatch=docomparison, multimatch_grouping=g)
    plain2, none2 = evaluation(gt2, pred2), evaluation(gt2, pred2, multimatch_grouping=None)
    for part in (0, 1):
        for grp in ("MultiMatch", "ScanMatch", "VAME"):
            for key, v in host2[part][grp].items():
                assert abs(float(dev2[part][grp][key]) - float(v)) <= 1e-6, (part, grp, key)
                assert _same(none2[part][grp][key], plain2[part][grp][key])
    for a, b in zip(dev2[2], host2[2]):
        assert np.allclose(a, b, rtol=0, atol=1e-9)
    assert all(np.array_equal(a, b) for a, b in zip(none2[2], plain2[2]))
