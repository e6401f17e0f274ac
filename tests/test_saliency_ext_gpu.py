"""Shuffled AUC, CC, SIM and information gain on the device (csrc/salmaps.hip sp_fixation_pool_counts / sp_saliency_scores,
visual_attention_metrics.saliency_scores_pairs, saliency_maps.scanpath_saliency, evaluation.saliency_*evaluation) against the numpy
checker tests/saliency_ext_ref.py, fed the identical float64 inputs.

Bars.  sAUC: bit-equal -- both sides divide the same two integers.  CC and SIM: 1e-12 absolute, IG: 1e-12 x max(1, |ref|) -- numpy's
pairwise sums against 256 strided sums and a fixed tree differ by <= 8e-16 at P = 76 800 (measured on the host), so the bar leaves the
project's usual x30 or more over summation-order noise; log2 differs in the last bit, 2^-53 x 52 bits per term at most.  The NaN
pattern is identical.  Repeats, batch against single maps and device against host inputs: bit-identical.  End to end (device
rasterisation and blur against a numpy pixel rule and scipy.ndimage.gaussian_filter): 1e-9, as tests/test_fixmaps_gpu.py.

The end-to-end generator keeps a gap for sAUC, the condition tests/golden/make_golden_fixmaps.py uses for AUC-Judd: a case is refused
(next seed) when a threshold -- the predicted density at a human-fixated pixel -- has a POOL pixel's value closer than 1e-9 x the
map's maximum without being equal to it.  The device's density maps are within 1e-12 x max of scipy's and have the same exact
zeros, so below that gap no comparison can flip and sAUC can differ only by its final division."""
import numpy as np
import pytest
import torch
from scipy.ndimage import gaussian_filter

import saliency_ext_ref as R
from helpers import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = ("sAUC", "CC", "SIM", "IG")


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def _reference(S, F, D, B, w, mix, brute=False):
    return {"sAUC": np.array([R.sauc(s, f, ww, brute=brute) for s, f, ww in zip(S, F, w)]),
            "CC": np.array([R.cc(s, d) for s, d in zip(S, D)]), "SIM": np.array([R.sim(s, d) for s, d in zip(S, D)]),
            "IG": np.array([R.infogain(s, f, b, mix) for s, f, b in zip(S, F, B)])}


def _compare(tag, got, ref, bar=1e-12, auc_exact=True):
    worst = {}
    for m in ALL:
        g = got[m].cpu().numpy() if isinstance(got[m], torch.Tensor) else np.asarray(got[m])
        r = ref[m]
        assert g.shape == r.shape, (tag, m, g.shape, r.shape)
        assert np.array_equal(np.isnan(g), np.isnan(r)), (tag, m, "NaN pattern", g, r)
        ok = ~np.isnan(r)
        scale = np.maximum(1.0, np.abs(r[ok])) if m == "IG" else 1.0
        worst[m] = float(np.max(np.abs(g[ok] - r[ok]) / scale)) if ok.any() else 0.0
    print(f"{tag}: " + ", ".join(f"{m} {worst[m]:.2e}" for m in ALL))
    for m in ALL:
        if m == "sAUC" and auc_exact:
            g = got[m].cpu().numpy()
            assert np.array_equal(g.view(np.int64)[~np.isnan(g)], ref[m].view(np.int64)[~np.isnan(g)]), (tag, "sAUC must be bit-equal", worst[m])
        else:
            assert worst[m] <= bar, (tag, m, worst[m])
    return worst


def _fixations(g, shape, n):
    f = np.zeros(shape)
    f.reshape(-1)[g.choice(f.size, n, replace=False)] = 1.0
    return f


def _op_set(g, N, H, W, kind, nfix):
    """N maps: kind 'random' (uniform), 'blurred' (Gaussian-filtered sparse counts, exact zeros included) or 'levels' (9 values)"""
    def one():
        if kind == "random":
            return g.uniform(0, 1, (H, W))
        if kind == "levels":
            return np.floor(g.uniform(0, 1, (H, W)) * 9) / 9
        c = np.zeros((H, W))
        np.add.at(c.reshape(-1), g.choice(H * W, 40), 1.0)
        return gaussian_filter(c, H / 24.0, mode="constant", cval=0.0, truncate=4.0)
    S, D, B = (np.stack([one() for _ in range(N)]) for _ in range(3))
    F = np.stack([_fixations(g, (H, W), nfix[k % len(nfix)]) * g.integers(1, 4, (H, W)) for k in range(N)])
    return S, F, D, B


def _run_pooled(S, F, D, B, cls, mix):
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    got = M.saliency_scores_pairs(S, F, D, B, image_groups=cls, uniform_mix=mix)
    assert sorted(got) == sorted(ALL) and all(v.is_cuda and v.dtype == torch.float64 and tuple(v.shape) == (len(S),) for v in got.values())
    cnt, tot = R.pool_counts(F, cls, max(cls) + 1)
    return got, R.pool_weights(cnt, tot, cls)


def test_scores_match_the_checker():
    from scanpaths_amd import hip
    g = np.random.Generator(np.random.PCG64(41))
    lds = hip.lib().sp_saliency_metrics_lds_fixations()
    n = 0
    for (H, W), N, sizes in (((30, 40), 6, (12, 1, 40)), ((240, 320), 4, (60, lds + 500, 7))):
        for kind in ("random", "blurred", "levels"):
            for mix in (0.0, 0.01):
                S, F, D, B = _op_set(g, N, H, W, kind, sizes)
                cls = [k % 3 for k in range(N)]
                if (H, W) == (240, 320):
                    assert (F.reshape(N, -1) > 0).sum(1).max() > lds                 # the global-scratch path runs
                got, w = _run_pooled(S, F, D, B, cls, mix)
                ref = _reference(S, F, D, B, w, mix, brute=(H, W) == (30, 40))
                assert not any(np.isnan(v).any() for v in ref.values()), "no NaN outside the cases built for it"
                _compare(f"{kind} {H}x{W} mix {mix}", got, ref)
                n += 1
    assert n == 12


def test_nan_cases_are_the_checkers():
    """NaN on purpose: no fixation, an empty pool, all groups on one image, a zero-sum map, a NaN pixel -- and nowhere else"""
    g = np.random.Generator(np.random.PCG64(43))
    H, W, N = 30, 40, 6
    S, F, D, B = _op_set(g, N, H, W, "blurred", (15,))
    F[0] = 0.0                                     # no fixation: sAUC and IG
    S[1] = 0.0                                     # a zero-sum prediction: CC, SIM and IG, while sAUC is 0.5
    S[2, 4, 5] = np.nan                            # a NaN pixel: all four
    D[3] = 0.0                                     # a zero-sum human density: CC and SIM
    B[4] = 0.0                                     # a zero-sum baseline: IG
    cls = [0, 1, 2, 0, 1, 2]
    got, w = _run_pooled(S, F, D, B, cls, 0.0)
    ref = _reference(S, F, D, B, w, 0.0, brute=True)
    expect = {"sAUC": [1, 0, 1, 0, 0, 0], "CC": [0, 1, 1, 1, 0, 0], "SIM": [0, 1, 1, 1, 0, 0], "IG": [1, 1, 1, 0, 1, 0]}
    for m in ALL:
        assert np.isnan(ref[m]).astype(int).tolist() == expect[m], (m, ref[m])
    assert ref["sAUC"][1] == 0.5
    _compare("NaN cases", got, ref)
    # a mixing weight does not change which cases are NaN: the sums decide
    got, w = _run_pooled(S, F, D, B, cls, 0.5)
    _compare("NaN cases, mix 0.5", got, _reference(S, F, D, B, w, 0.5))
    # all groups on one image: nobody has a pool
    S, F, D, B = _op_set(g, 4, H, W, "random", (15,))
    got, w = _run_pooled(S, F, D, B, [0, 0, 0, 0], 0.01)
    assert not w.any()
    ref = _reference(S, F, D, B, w, 0.01)
    assert np.isnan(ref["sAUC"]).all() and not any(np.isnan(ref[m]).any() for m in ("CC", "SIM", "IG"))
    _compare("one image", got, ref)
    # an empty pool: the only other image has no fixation
    F[3] = 0.0
    got, w = _run_pooled(S, F, D, B, [0, 0, 0, 1], 0.01)
    assert not w[:3].any() and w[3].any()
    ref = _reference(S, F, D, B, w, 0.01)
    assert np.isnan(ref["sAUC"]).all()
    _compare("empty pool", got, ref)


def test_repeats_batching_and_device_inputs_are_bitwise():
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    g = np.random.Generator(np.random.PCG64(47))
    lds = hip.lib().sp_saliency_metrics_lds_fixations()
    for (H, W), N, sizes in (((30, 40), 5, (9, 30)), ((240, 320), 3, (lds + 100, 50))):
        S, F, D, B = _op_set(g, N, H, W, "blurred", sizes)
        F[-1] = 0.0
        cls = [0, 1, 2, 1, 0][:N]
        a, w = _run_pooled(S, F, D, B, cls, 0.01)
        b, _ = _run_pooled(S, F, D, B, cls, 0.01)
        for m in ALL:
            assert torch.equal(_bits(a[m]), _bits(b[m])), (m, "two calls")
        # the pool given as explicit weight maps, and the per-map wrappers (one upload and launch each)
        c = M.saliency_scores_pairs(S, F, D, B, other_maps=w, uniform_mix=0.01)
        for m in ALL:
            assert torch.equal(_bits(a[m]), _bits(c[m])), (m, "image_groups against other_maps")
        one = {"sAUC": [M.AUC_shuffled(S[k], F[k], w[k]) for k in range(N)], "CC": [M.CC(S[k], D[k]) for k in range(N)],
               "SIM": [M.SIM(S[k], D[k]) for k in range(N)], "IG": [M.InfoGain(S[k], F[k], B[k], uniform_mix=0.01) for k in range(N)]}
        for m in ALL:
            assert all(isinstance(v, float) for v in one[m])
            assert np.array_equal(np.array(one[m]).view(np.int64), a[m].cpu().numpy().view(np.int64)), (m, "batch against wrappers")
        # device tensors are used in place and give the same bits; so do non-contiguous views
        Sd, Fd, Dd, Bd = (torch.from_numpy(x).to(DEV) for x in (S, F, D, B))
        d = M.saliency_scores_pairs(Sd, Fd, Dd, Bd, image_groups=cls, uniform_mix=0.01)
        e = M.saliency_scores_pairs(Sd, Fd, Dd, Bd, other_maps=torch.from_numpy(w).to(DEV), uniform_mix=0.01)
        Sp = torch.zeros((N, H, W + 3), dtype=torch.float64, device=DEV)
        Sp[:, :, :W] = Sd
        f = M.saliency_scores_pairs(Sp[:, :, :W], F, Dd, B, image_groups=torch.tensor(cls), uniform_mix=0.01)
        for m in ALL:
            assert torch.equal(_bits(a[m]), _bits(d[m])) and torch.equal(_bits(a[m]), _bits(e[m])) and torch.equal(_bits(a[m]), _bits(f[m])), m
    # only what the inputs allow, one launch per entry point
    calls = {}
    L = hip.lib()
    orig = {n: getattr(L, n) for n in ("sp_saliency_scores", "sp_fixation_pool_counts", "sp_count_positive")}
    for n, fn in orig.items():
        def counted(*args, _n=n, _fn=fn):
            calls[_n] = calls.get(_n, 0) + 1
            return _fn(*args)
        setattr(L, n, counted)
    try:
        assert sorted(M.saliency_scores_pairs(Sd, density_maps=Dd)) == ["CC", "SIM"] and calls == {"sp_saliency_scores": 1}
        assert sorted(M.saliency_scores_pairs(Sd, Fd, baseline_maps=Bd, uniform_mix=0.0)) == ["IG"]
        calls.clear()
        assert sorted(M.saliency_scores_pairs(Sd, Fd, image_groups=cls)) == ["sAUC"]
        assert calls == {"sp_saliency_scores": 1, "sp_fixation_pool_counts": 1, "sp_count_positive": 1}
    finally:
        for n, fn in orig.items():
            setattr(L, n, fn)
    with pytest.raises(ValueError, match="integers"):
        M.saliency_scores_pairs(Sd, Fd, other_maps=torch.from_numpy(w + 0.5).to(DEV))
    assert all(tuple(v.shape) == (0,) for v in M.saliency_scores_pairs(S[:0], F[:0], D[:0], B[:0], image_groups=[], uniform_mix=0.0).values())


# ---- scanpath level ------------------------------------------------------------------------------------------------------------------
FRAME = (240.0, 320.0)


def _rasterise(paths, groups, G, shape):
    """the pixel rule of include/scanpaths_amd.h sp_fixation_maps in numpy: (binary, count) [G,H,W]"""
    H, W = shape
    count = np.zeros((G, H, W))
    for p, q in zip(paths, groups):
        for x, y in np.asarray(p, dtype=np.float64).reshape(-1, 3)[:, :2]:
            if not (np.isfinite(x) and np.isfinite(y)) or x < 0 or x >= FRAME[1] or y < 0 or y >= FRAME[0]:
                continue
            count[q, min(int(np.floor(y * H / FRAME[0])), H - 1), min(int(np.floor(x * W / FRAME[1])), W - 1)] += 1.0
    return (count > 0).astype(np.float64), count


def _blur(m, sigma, mode):
    return np.stack([gaussian_filter(x, sigma, mode=mode, cval=0.0, truncate=4.0) for x in m]) if len(m) else m


def _gap(S, F, w):
    """the smallest non-zero distance of a threshold to a pool pixel's value, relative to the map's maximum (inf: no such pair)"""
    v = np.sort(S[w > 0])
    gap = np.inf
    if not v.size or not S.max() > 0:
        return gap
    for t in S[F > 0]:
        i, j = np.searchsorted(v, t, "left"), np.searchsorted(v, t, "right")
        if i > 0:
            gap = min(gap, t - v[i - 1])
        if j < v.size:
            gap = min(gap, v[j] - t)
    return gap / S.max()


def _host_scores(gt, gt_g, pr, pr_g, cls, G, shape, sigma, mode, mix, centre=False):
    """(metric -> [G], smallest sAUC gap): checker-side pool counts, scipy blur and the checker's metrics"""
    E = max(cls) + 1
    b, c = _rasterise(gt, gt_g, G, shape)
    _, pc = _rasterise(pr, pr_g, G, shape)
    D = _blur(c, sigma, mode)
    per_image = np.stack([sum((c[q] for q in range(G) if cls[q] == e), np.zeros(shape)) for e in range(E)])
    Bi = _blur(per_image.sum(0)[None] - per_image, sigma, mode)
    B = np.stack([Bi[cls[q]] for q in range(G)])
    S = B if centre else _blur(pc, sigma, mode)
    cnt, tot = R.pool_counts(b, cls, E)
    w = R.pool_weights(cnt, tot, cls)
    with np.errstate(all="ignore"):
        return _reference(S, b, D, B, w, mix), min(_gap(S[q], b[q], w[q]) for q in range(G))


def _nanmean_rows(folds, members, nkeys):
    out = {m: np.full(nkeys, np.nan) for m in ALL}
    for q, mem in enumerate(members):
        if len(mem) >= 2:
            for m in ALL:
                v = folds[m][mem]
                if not np.isnan(v).all():
                    out[m][q] = np.nanmean(v)
    return out


def _paths(g, n, lo=3, hi=10):
    return [np.stack([g.uniform(0, FRAME[1], k), g.uniform(0, FRAME[0], k), g.uniform(0.08, 0.6, k)], 1)
            for k in (int(g.integers(lo, hi + 1)) for _ in range(n))]


def _e2e_case(seed, shape, sigma, mode, mix):
    """7 questions on 3 images: 2-5 human scanpaths each (question 5: one), 8 predicted each (question 6: none).  None when a
    comparison of sAUC could flip in one of the three rows."""
    g = np.random.Generator(np.random.PCG64(seed))
    G = 7
    img_of = [0, 1, 2, 0, 1, 2, 0]
    gt, keys, pr, pkeys = [], [], [], []
    for q in range(G):
        nh = 1 if q == 5 else int(g.integers(2, 6))
        gt += _paths(g, nh)
        keys += [q] * nh
        if q != 6:
            pr += _paths(g, 8)
            pkeys += [q] * 8
    order = g.permutation(len(gt))                                        # keys interleaved: first-appearance order is not sorted
    gt, keys = [gt[k] for k in order], [keys[k] for k in order]
    names = {}
    for k in keys:
        names.setdefault(k, len(names))
    gt_g, pr_g = [names[k] for k in keys], [names[k] for k in pkeys]
    cls = [0] * G
    for k, q in names.items():
        cls[q] = img_of[k]
    model, g1 = _host_scores(gt, gt_g, pr, pr_g, cls, G, shape, sigma, mode, mix)
    floor, g2 = _host_scores(gt, gt_g, [], [], cls, G, shape, sigma, mode, mix, centre=True)
    # the ceiling: fold i holds scanpath i out, the other scanpaths of its question predict it
    members = [[i for i, q in enumerate(gt_g) if q == k] for k in range(G)]
    fp, fg = [], []
    for i, q in enumerate(gt_g):
        for j in members[q]:
            if j != i:
                fp.append(gt[j])
                fg.append(i)
    folds, g3 = _host_scores(gt, list(range(len(gt))), fp, fg, [cls[q] for q in gt_g], len(gt), shape, sigma, mode, mix)
    if min(g1, g2, g3) < 1e-9:
        return None
    return dict(gt=gt, keys=[f"q{k}" for k in keys], pr=pr, pkeys=[f"q{k}" for k in pkeys], images=[f"img{img_of[k]}" for k in keys],
                order=[f"q{k}" for k in names], model=model, floor=floor, human=_nanmean_rows(folds, members, G), gap=min(g1, g2, g3), cls=cls)


def _check_rows(tag, means, per_key, ref):
    worst = _compare(tag, {m: per_key[m] for m in ALL}, ref, bar=1e-9, auc_exact=False)
    for m in ALL:
        nan = np.isnan(ref[m])
        assert means[m + "_nan"] == int(nan.sum()), (tag, m)
        if (~nan).any():
            assert abs(means[m] - ref[m][~nan].mean()) <= 1e-9 * max(1.0, abs(ref[m][~nan].mean())), (tag, m)
        else:
            assert np.isnan(means[m])
    return worst


def test_evaluation_ceiling_and_floor_match_a_host_composition():
    from scanpaths_amd.utils import evaluation as E
    n = 0
    for shape, sigma, mode, mix in (((30, 40), 1.5, "constant", 0.01), ((60, 80), 2.5, "reflect", 0.0), ((240, 320), 10.0, "constant", 0.05)):
        case = next(c for c in (_e2e_case(seed, shape, sigma, mode, mix) for seed in range(100, 200)) if c is not None)
        kw = dict(sigma=sigma, extra_metrics=ALL, image_keys=case["images"], uniform_mix=mix, output_shape=shape, mode=mode)
        tag = f"{shape} sigma {sigma} {mode} (gap {case['gap']:.1e})"
        means, per_key = E.saliency_evaluation(case["gt"], case["pr"], case["keys"], case["pkeys"], **kw)
        assert per_key["keys"] == case["order"]
        assert set(means) == {m + s for m in ("AUC_Judd", "NSS", "KLdiv") + ALL for s in ("", "_nan")}
        _check_rows("model " + tag, means, per_key, case["model"])
        hm, hk = E.saliency_human_evaluation(case["gt"], case["keys"], **kw)
        assert hk["keys"] == case["order"] and set(hm) == set(means)
        _check_rows("human " + tag, hm, hk, case["human"])
        single = case["order"].index("q5")
        assert all(np.isnan(hk[m][single]) for m in ("AUC_Judd", "NSS", "KLdiv") + ALL) and hm["sAUC_nan"] >= 1   # one scanpath: NaN, counted
        cm, ck = E.saliency_centre_prior_evaluation(case["gt"], case["keys"], **kw)
        assert ck["keys"] == case["order"]
        _check_rows("centre prior " + tag, cm, ck, case["floor"])
        assert (ck["IG"] == 0.0).all() and not np.signbit(ck["IG"]).any(), "every key has a pool here: exactly 0"
        n += 1
    assert n == 3
    # without image_keys every key is its own image; all keys on one image leave no pool and no baseline
    case = next(c for c in (_e2e_case(seed, (30, 40), 1.5, "constant", 0.01) for seed in range(100, 200)) if c is not None)
    kw = dict(sigma=1.5, extra_metrics=ALL, uniform_mix=0.01, output_shape=(30, 40))
    a = E.saliency_evaluation(case["gt"], case["pr"], case["keys"], case["pkeys"], **kw)[1]
    b = E.saliency_evaluation(case["gt"], case["pr"], case["keys"], case["pkeys"], image_keys=case["keys"], **kw)[1]
    for m in ALL:
        assert np.array_equal(a[m].view(np.int64), b[m].view(np.int64)), m
    cm, ck = E.saliency_centre_prior_evaluation(case["gt"], case["keys"], image_keys=["same"] * len(case["keys"]), **kw)
    assert np.isnan(ck["IG"]).all() and np.isnan(ck["sAUC"]).all() and cm["IG_nan"] == 7 and np.isnan(cm["IG"])


def test_defaults_are_unchanged_and_extras_leave_the_shared_metrics_alone():
    """without extras: today's keys, and the bits the same call gives with extras on AUC_Judd / NSS / KLdiv; the golden end-to-end
    cases of tests/test_fixmaps_gpu.py hold with the extras switched on"""
    import os
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    gold = load_npz(os.path.join(GOLDEN, "fixmaps.npz"))

    def paths(prefix):
        fix, lens = gold[prefix + "fix"], gold[prefix + "len"]
        off = np.concatenate([[0], np.cumsum(lens)])
        return [fix[off[k]:off[k + 1]] for k in range(len(lens))], [int(v) for v in gold[prefix + "group"]]

    n = 0
    for i, (shape, sigma) in enumerate(zip(gold["e2e/shapes"], gold["e2e/sigmas"])):
        shape = (int(shape[0]), int(shape[1]))
        for j, mode in enumerate(("constant", "reflect")):
            p = f"e2e/{i}/{j}/"
            gt, gt_g = paths(p + "gt_")
            pr, pr_g = paths(p + "pred_")
            plain = M.scanpath_saliency(gt, gt_g, pr, pr_g, (240, 320), float(sigma), output_shape=shape, mode=mode)
            assert sorted(plain) == ["AUC_Judd", "KLdiv", "NSS", "gt_dropped", "pred_dropped"]
            for extra, kw in ((ALL, dict(uniform_mix=0.01, image_groups=[0, 1, 0, 1, 2])), (("sAUC",), {}), (("CC", "IG"), dict(uniform_mix=0.0)),
                              (ALL, dict(uniform_mix=0.5, baseline_sigma=2.0 * float(sigma)))):
                full = M.scanpath_saliency(gt, gt_g, pr, pr_g, (240, 320), float(sigma), output_shape=shape, mode=mode, extra_metrics=extra, **kw)
                assert sorted(full) == sorted(list(plain) + list(extra))
                for k in ("AUC_Judd", "NSS", "KLdiv"):
                    assert torch.equal(_bits(plain[k]), _bits(full[k])), (p, k, extra)
                assert torch.equal(plain["gt_dropped"], full["gt_dropped"]) and torch.equal(plain["pred_dropped"], full["pred_dropped"])
                assert all(full[m].is_cuda and full[m].dtype == torch.float64 and tuple(full[m].shape) == (5,) for m in extra)
            for res in (plain, full):
                for k, r in (("AUC_Judd", gold[p + "auc"]), ("NSS", gold[p + "nss"]), ("KLdiv", gold[p + "kld"])):
                    v = res[k].cpu().numpy()
                    assert np.array_equal(np.isnan(v), np.isnan(r)), (p, k)
                    with np.errstate(all="ignore"):
                        err = np.nanmax(np.abs(v - r) / (np.where(r != 0, np.abs(r), 1.0) if k == "KLdiv" else 1.0))
                    assert err <= 1e-9, (p, k, err)
            names = [f"q{100 - q}" for q in range(5)]
            args = (gt, pr, [names[q] for q in gt_g], [names[q] for q in pr_g], (240, 320))
            m0, k0 = E.saliency_evaluation(*args, sigma=float(sigma), output_shape=shape, mode=mode)
            m1, k1 = E.saliency_evaluation(*args, sigma=float(sigma), output_shape=shape, mode=mode, extra_metrics=ALL, uniform_mix=0.01)
            assert sorted(m0) == sorted(m + s for m in ("AUC_Judd", "NSS", "KLdiv") for s in ("", "_nan"))
            assert sorted(k0) == ["AUC_Judd", "KLdiv", "NSS", "gt_dropped", "keys", "pred_dropped"]
            assert sorted(k1) == sorted(list(k0) + list(ALL)) and sorted(m1) == sorted(list(m0) + [m + s for m in ALL for s in ("", "_nan")])
            for k in k0:
                if k == "keys":
                    assert k0[k] == k1[k]
                else:
                    assert np.array_equal(k0[k].view(np.int64) if k0[k].dtype == np.float64 else k0[k],
                                          k1[k].view(np.int64) if k1[k].dtype == np.float64 else k1[k]), k
            for k in m0:
                assert m0[k] == m1[k] or (np.isnan(m0[k]) and np.isnan(m1[k])), k
            n += 1
    assert n >= 6


def test_costs_do_not_depend_on_the_number_of_keys():
    """entry-point calls (= launches) and device-to-host copies of a saliency_evaluation / ceiling / floor call with all extras"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils import evaluation as E
    L = hip.lib()
    names = ("sp_fixation_maps", "sp_gaussian_blur_maps", "sp_count_positive", "sp_saliency_metrics", "sp_fixation_pool_counts",
             "sp_saliency_scores")
    seen = []
    for G in (3, 11):
        g = np.random.Generator(np.random.PCG64(G))
        gt, keys, pr, pkeys = [], [], [], []
        for q in range(G):
            gt += _paths(g, 3)
            keys += [q] * 3
            pr += _paths(g, 4)
            pkeys += [q] * 4
        calls, copies = {}, [0]
        orig = {n: getattr(L, n) for n in names}
        for n, fn in orig.items():
            def counted(*args, _n=n, _fn=fn):
                calls[_n] = calls.get(_n, 0) + 1
                return _fn(*args)
            setattr(L, n, counted)
        cpu = torch.Tensor.cpu

        def counting_cpu(self, *a, **k):
            copies[0] += int(self.is_cuda)
            return cpu(self, *a, **k)
        torch.Tensor.cpu = counting_cpu
        try:
            kw = dict(sigma=1.5, output_shape=(30, 40), extra_metrics=ALL, uniform_mix=0.01, image_keys=[q % 3 for q in keys])
            rec = []
            for fn, args in ((E.saliency_evaluation, (gt, pr, keys, pkeys)), (E.saliency_human_evaluation, (gt, keys)),
                             (E.saliency_centre_prior_evaluation, (gt, keys))):
                calls.clear()
                copies[0] = 0
                fn(*args, **kw)
                rec.append((dict(calls), copies[0]))
        finally:
            torch.Tensor.cpu = cpu
            for n, fn in orig.items():
                setattr(L, n, fn)
        seen.append(rec)
    print("entry-point calls and device-to-host copies per call (model, human, centre prior):", seen[0])
    assert seen[0] == seen[1]
    assert seen[0][0][0] == {"sp_fixation_maps": 3, "sp_gaussian_blur_maps": 2, "sp_count_positive": 1, "sp_saliency_metrics": 2,
                             "sp_fixation_pool_counts": 1, "sp_saliency_scores": 1}


def test_new_entry_points_error_codes():
    """unsupported arguments -> SP_EINVAL, null buffers -> SP_ENULL: never a crash, never a silent fallback"""
    from scanpaths_amd import hip
    L = hip.lib()
    st = hip.stream()
    N, P, E = 3, 64, 2
    g = np.random.Generator(np.random.PCG64(3))
    Sn, Fn = g.uniform(0, 1, (N, P)), (g.uniform(0, 1, (N, P)) < 0.2).astype(np.float64)
    S, F = torch.from_numpy(Sn).to(DEV), torch.from_numpy(Fn).to(DEV)
    cls = np.array([0, 1, 0], dtype=np.int32)
    cls_d = torch.full((N,), -5, dtype=torch.int32, device=DEV)
    cnt = torch.full((E, P), -7, dtype=torch.int32, device=DEV)
    tot = torch.full((P,), -7, dtype=torch.int32, device=DEV)
    p = hip.ptr
    assert L.sp_fixation_pool_counts(p(F), cls.ctypes.data, N, P, E, p(cls_d), p(cnt), p(tot), st) == 0
    rc, rt = R.pool_counts(Fn, cls, E)
    assert np.array_equal(cnt.cpu().numpy(), rc) and np.array_equal(tot.cpu().numpy(), rt) and cls_d.tolist() == [0, 1, 0]
    for bad in ([0, 2, 0], [0, -1, 0]):                                       # an image outside [0, E): checked on the host
        b = np.array(bad, dtype=np.int32)
        assert L.sp_fixation_pool_counts(p(F), b.ctypes.data, N, P, E, p(cls_d), p(cnt), p(tot), st) == -1
    assert cls_d.tolist() == [0, 1, 0], "a refused call launches nothing"
    for args in ((0, P, E), (N, 0, E), (N, P, 0)):
        assert L.sp_fixation_pool_counts(p(F), cls.ctypes.data, *args, p(cls_d), p(cnt), p(tot), st) == -1
    assert L.sp_fixation_pool_counts(None, cls.ctypes.data, N, P, E, p(cls_d), p(cnt), p(tot), st) == -2
    assert L.sp_fixation_pool_counts(p(F), None, N, P, E, p(cls_d), p(cnt), p(tot), st) == -2
    assert L.sp_fixation_pool_counts(p(F), cls.ctypes.data, N, P, E, None, p(cnt), p(tot), st) == -2
    assert L.sp_fixation_pool_counts(p(F), cls.ctypes.data, N, P, E, p(cls_d), None, p(tot), st) == -2
    assert L.sp_fixation_pool_counts(p(F), cls.ctypes.data, N, P, E, p(cls_d), p(cnt), None, st) == -2

    off = torch.zeros(N + 1, dtype=torch.int64, device=DEV)
    out = [torch.full((N,), -3.0, dtype=torch.float64, device=DEV) for _ in range(4)]

    def scores(sal=S, fix=F, dens=S, base=S, pool=tot, stride=0, cnt_=cnt, cls_=cls_d, E_=E, N_=N, P_=P, mix=0.0, off_=off, outs=None):
        o = out if outs is None else outs
        return L.sp_saliency_scores(p(sal), p(fix), p(dens), p(base), p(pool), stride, p(cnt_), p(cls_), E_, N_, P_, mix, p(off_), None,
                                    p(o[0]), p(o[1]), p(o[2]), p(o[3]), st)

    assert scores() == 0
    w = R.pool_weights(rc, rt, cls)
    ref = _reference(Sn, Fn, Sn, Sn, w, 0.0, brute=True)
    _compare("C ABI", dict(zip(ALL, out)), ref)
    assert (out[3] == 0.0).all() and float(out[2][0]) == pytest.approx(1.0, abs=1e-12)       # S against itself
    assert scores(N_=0) == -1 and scores(P_=0) == -1
    assert scores(mix=-0.1) == -1 and scores(mix=1.5) == -1 and scores(mix=float("nan")) == -1
    assert scores(stride=7) == -1 and scores(E_=0) == -1
    assert scores(sal=None) == -2 and scores(cnt_=None) == -2 and scores(cls_=None) == -2 and scores(off_=None) == -2
    assert scores(outs=[None] * 4) == -2                                                     # nothing to compute
    assert scores(fix=None, dens=None) == -2                                                 # every requested metric lacks an input
    # a NULL input or output skips that metric and leaves its output alone
    for o in out:
        o.fill_(-3.0)
    assert scores(fix=None) == 0 and (out[0] == -3.0).all() and (out[3] == -3.0).all() and not (out[1] == -3.0).any()
    for o in out:
        o.fill_(-3.0)
    assert scores(dens=None, base=None, outs=[out[0], None, out[2], out[3]]) == 0
    assert not (out[0] == -3.0).any() and (out[2] == -3.0).all() and (out[3] == -3.0).all()
    # explicit weight maps: pool [N][P], no cnt / cls; a stray image index on the device scores NaN instead of reading outside cnt
    wd = torch.from_numpy(w.astype(np.int32)).to(DEV)
    assert scores(pool=wd, stride=P, cnt_=None, cls_=None, E_=0) == 0
    assert np.array_equal(out[0].cpu().numpy().view(np.int64), ref["sAUC"].view(np.int64))
    stray = torch.tensor([0, 9, -1], dtype=torch.int32, device=DEV)
    assert scores(cls_=stray) == 0
    v = out[0].cpu().numpy()
    assert not np.isnan(v[0]) and np.isnan(v[1:]).all()
    with pytest.raises(hip.HipError):
        hip.check(scores(mix=2.0), "sp_saliency_scores")
