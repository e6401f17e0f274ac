"""Fixation maps, density maps and the saliency scoring of scanpaths on the device (csrc/fixmaps.hip, evaltools/saliency_maps.py)
against tests/golden/fixmaps.npz (tests/golden/make_golden_fixmaps.py: a numpy loop with the pixel rule, scipy.ndimage.gaussian_filter
and the REAL reference's AUC_Judd(jitter=False) / NSS / KLdiv on the scipy maps).

Bars.  Fixation maps and `dropped`: bit-exact, all three weights.  Density maps: 1e-12 x max|ref| per map -- two passes of at most
2 * 64 + 1 non-negative terms give <= 2 * 129 * 2^-53 ~ 3e-14 relative, so the bar leaves x30; exact zeros match exactly (the support
is the same box of the truncated kernel).  Repeats and batch-vs-single: bit-identical.  saliency_metrics_pairs on device tensors:
bitwise the numpy call.  End to end: AUC within 1e-9 (the generator's gap condition rules out an order flip under the map bar), NSS
within 1e-9 absolute, KLdiv within 1e-9 relative, NaN rows identical."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODES = ("constant", "reflect", "nearest")
FV = {"names": ("start_x", "start_y", "duration"), "formats": ("f8", "f8", "f8")}


@pytest.fixture(scope="module")
def gold():
    return load_npz(os.path.join(GOLDEN, "fixmaps.npz"))


def _paths(g, prefix):
    fix, lens = g[prefix + "fix"], g[prefix + "len"]
    off = np.concatenate([[0], np.cumsum(lens)])
    return [fix[off[k]:off[k + 1]] for k in range(len(lens))], [int(v) for v in g[prefix + "group"]]


def _expected(g, k, G, shape):
    out = {}
    for w in ("binary", "count", "duration"):
        v = g[f"fm/{k}/{w}"]
        if f"fm/{k}/nz" in g:
            full = np.zeros(G * shape[0] * shape[1])
            full[g[f"fm/{k}/nz"]] = v
            v = full.reshape(G, *shape)
        out[w] = v
    return out


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64)


def test_fixation_maps_are_bit_exact(gold):
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    paths, groups = _paths(gold, "fm/")
    frame = tuple(float(v) for v in gold["fm/frame"])
    G = 5
    L = hip.lib()
    assert max(len(p) for p in paths) > L.sp_scan_max_fixations()                 # that limit does not apply here
    # C ABI: one upload of the concatenated rows
    fix = torch.from_numpy(gold["fm/fix"]).to(DEV)
    lens = gold["fm/len"]
    start = torch.from_numpy(np.cumsum(lens) - lens).to(DEV)
    count = torch.from_numpy(lens.astype(np.int32)).to(DEV)
    grp = torch.from_numpy(gold["fm/group"].astype(np.int32)).to(DEV)
    for k, shape in enumerate(gold["fm/shapes"]):
        H, W = int(shape[0]), int(shape[1])
        exp = _expected(gold, k, G, (H, W))
        for wi, w in enumerate(("binary", "count", "duration")):
            maps = torch.full((G, H, W), -7.0, dtype=torch.float64, device=DEV)
            dropped = torch.full((G,), -1, dtype=torch.int32, device=DEV)
            rc = L.sp_fixation_maps(hip.ptr(fix), 3, hip.ptr(start), hip.ptr(count), hip.ptr(grp), len(lens), G, H, W, frame[1], frame[0], wi,
                                    hip.ptr(maps), hip.ptr(dropped), hip.stream())
            assert rc == 0
            assert np.array_equal(maps.cpu().numpy().view(np.int64), exp[w].view(np.int64)), (k, w, "C ABI")
            assert np.array_equal(dropped.cpu().numpy(), gold[f"fm/{k}/dropped"]), (k, w)
            m2, d2 = M.fixation_maps(paths, groups, frame, output_shape=None if (H, W) == (240, 320) else (H, W), weight=w)
            assert m2.dtype == torch.float64 and m2.is_cuda and tuple(m2.shape) == (G, H, W) and d2.dtype == torch.int32
            assert torch.equal(_bits(m2), _bits(maps)) and torch.equal(d2, dropped), (k, w, "fixation_maps")
            m3, _ = M.fixation_maps(paths, groups, frame, output_shape=(H, W), weight=w)            # a second call: the same bits
            assert torch.equal(_bits(m3), _bits(m2))
    # structured fixation vectors and plain arrays are the same input
    fvs = []
    for p in paths:
        a = np.zeros(len(p), dtype=FV)
        a["start_x"], a["start_y"], a["duration"] = p[:, 0], p[:, 1], p[:, 2]
        fvs.append(a)
    a, da = M.fixation_maps(fvs, groups, frame, output_shape=(30, 40), weight="duration")
    b, db = M.fixation_maps(paths, groups, frame, output_shape=(30, 40), weight="duration")
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(da, db)
    # num_groups beyond the last used group: zero maps
    m, d = M.fixation_maps(paths, groups, frame, output_shape=(30, 40), num_groups=7)
    assert tuple(m.shape) == (7, 30, 40) and not m[5:].any() and not d[5:].any() and not m[3].any()
    # rounding up to col == W is clamped to the last pixel
    cp, cg = _paths(gold, "fmclamp/")
    H, W = (int(v) for v in gold["fmclamp/shape"])
    m, d = M.fixation_maps(cp, cg, tuple(gold["fmclamp/frame"]), output_shape=(H, W), weight="count")
    assert np.array_equal(m.cpu().numpy(), gold["fmclamp/count"]) and int(d[0]) == 0 and m[0, 1, W - 1] == 1


def _density_err(out, ref):
    out = out.cpu().numpy()
    errs = []
    for o, r in zip(out, ref):
        scale = np.abs(r).max()
        errs.append(np.abs(o - r).max() / scale if scale else np.abs(o).max())
        assert np.array_equal(o == 0, r == 0), "exact zeros must match"
    return max(errs)


def test_density_maps_match_scipy(gold):
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    params = gold["blur/params"]
    worst = 0.0
    for tag in ("30x40", "40x64"):
        x = gold[f"blur/{tag}/in"]
        xd = torch.from_numpy(x).to(DEV)
        for mode in MODES:
            for k, (sy, sx, tr) in enumerate(params):
                ref = gold[f"blur/{tag}/{mode}/{k}"]
                out = M.density_maps(xd, (sy, sx), truncate=tr, mode=mode)
                assert out.is_cuda and out.dtype == torch.float64 and out.shape == xd.shape
                err = _density_err(out, ref)
                print(f"density {tag} {mode} sigma ({sy}, {sx}) truncate {tr}: {err:.2e} of max")
                worst = max(worst, err)
                assert err <= 1e-12, (tag, mode, k, err)
                out2 = M.density_maps(x, (sy, sx), truncate=tr, mode=mode)                # host maps in, a second call: the same bits
                assert torch.equal(_bits(out2), _bits(out))
                one = torch.cat([M.density_maps(xd[i:i + 1], (sy, sx), truncate=tr, mode=mode) for i in range(x.shape[0])])
                assert torch.equal(_bits(one), _bits(out)), "a batch and its maps one at a time"
                if sy == sx:                                                             # a scalar sigma is (sigma, sigma)
                    assert torch.equal(_bits(M.density_maps(xd, float(sy), truncate=tr, mode=mode)), _bits(out))
    # normalisation: each map by its sum / max; a zero map stays zero
    x = torch.from_numpy(np.concatenate([gold["blur/30x40/in"], np.zeros((1, 30, 40))])).to(DEV)
    ref = np.concatenate([gold["blur/30x40/constant/0"], np.zeros((1, 30, 40))])
    for how, red in (("sum", lambda a: a.sum()), ("max", lambda a: a.max())):
        out = M.density_maps(x, 1.5, mode="constant", normalise=how).cpu().numpy()
        for o, r in zip(out[:-1], ref[:-1]):
            assert np.abs(o - r / red(r)).max() <= 1e-12 * np.abs(r / red(r)).max(), how
        assert not out[-1].any()
        assert abs(red(out[0]) - 1.0) <= 1e-12
    print(f"density worst {worst:.2e}")


def test_density_map_at_evaluation_size(gold):
    """240x320 at sigma 10 (81 taps per axis): a 4x-strided sample, the sum and the max of the scipy map"""
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    paths, groups = _paths(gold, "blur/big/")
    counts, dropped = M.fixation_maps(paths, groups, (240, 320), weight="count")
    assert int(dropped.sum()) == 0
    for mode in MODES:
        out = M.density_maps(counts, 10.0, mode=mode)
        o = out[0].cpu().numpy()
        ref, rmax, rsum = gold[f"blur/big/{mode}/sample"], float(gold[f"blur/big/{mode}/max"]), float(gold[f"blur/big/{mode}/sum"])
        err = np.abs(o[::4, ::4] - ref).max() / rmax
        print(f"density 240x320 sigma 10 {mode}: sample {err:.2e} of max, max {abs(o.max() - rmax) / rmax:.2e}, "
              f"sum {abs(o.sum() - rsum) / rsum:.2e}")
        assert err <= 1e-12 and abs(o.max() - rmax) <= 1e-12 * rmax
        # the sum: every pixel within the map bar, plus numpy's own pairwise rounding of 76800 terms (<= 17 levels x 2^-53)
        assert abs(o.sum() - rsum) <= 1e-12 * rmax * o.size + 2e-15 * rsum
        assert np.array_equal(o[::4, ::4] == 0, ref == 0)
        assert torch.equal(_bits(M.density_maps(counts, 10.0, mode=mode)), _bits(out))


def test_saliency_metrics_pairs_on_device_tensors_is_bitwise_the_numpy_call():
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    g = np.random.Generator(np.random.PCG64(31))
    lds = hip.lib().sp_saliency_metrics_lds_fixations()
    for (N, H, W), nfix in (((4, 30, 40), 15), ((3, 240, 320), lds + 500)):
        S = g.uniform(0, 1, (N, H, W))
        F = np.zeros((N, H, W))
        for n in range(N):
            F[n].reshape(-1)[g.choice(H * W, nfix if n else 3, replace=False)] = 1.0
        F[-1] = 0 if N == 4 else F[-1]                                         # a map without fixation: NaN rows
        J = g.uniform(0, 1e-7, (N, H, W))
        assert N == 4 or (F.reshape(N, -1) > 0).sum(1).max() > lds              # the global-scratch path runs
        for jit in (None, J):
            host = M.saliency_metrics_pairs(S, F, jit)
            Sd, Fd = torch.from_numpy(S).to(DEV), torch.from_numpy(F).to(DEV)
            dev = M.saliency_metrics_pairs(Sd, Fd, None if jit is None else torch.from_numpy(jit).to(DEV))
            for a, b in zip(host, dev):
                assert b.is_cuda and torch.equal(_bits(a), _bits(b))
            # non-contiguous device views are taken as they are
            Sp = torch.zeros((N, H, W + 3), dtype=torch.float64, device=DEV)
            Sp[:, :, :W] = Sd
            for a, b in zip(host, M.saliency_metrics_pairs(Sp[:, :, :W], Fd, jit)):
                assert torch.equal(_bits(a), _bits(b))
        # a float32 device tensor still goes the host way and gives what its numpy values give
        for a, b in zip(M.saliency_metrics_pairs(S.astype(np.float32), F), M.saliency_metrics_pairs(Sd.float(), Fd)):
            assert torch.equal(_bits(a), _bits(b))


def _check_scores(tag, got, gold, p):
    auc, nss, kld = (got[k] if isinstance(got[k], np.ndarray) else got[k].cpu().numpy() for k in ("AUC_Judd", "NSS", "KLdiv"))
    ra, rn, rk = gold[p + "auc"], gold[p + "nss"], gold[p + "kld"]
    with np.errstate(all="ignore"):
        ea, en = np.nanmax(np.abs(auc - ra)), np.nanmax(np.abs(nss - rn))
        ek = np.nanmax(np.abs(kld - rk) / np.where(rk != 0, np.abs(rk), 1.0))
    print(f"{tag}: AUC err {ea:.2e}, NSS err {en:.2e}, KLdiv rel err {ek:.2e} (gap {float(gold[p + 'gap']):.2e})")
    assert np.array_equal(np.isnan(auc), np.isnan(ra)) and np.array_equal(np.isnan(nss), np.isnan(rn))
    assert np.array_equal(np.isnan(kld), np.isnan(rk))
    assert ea <= 1e-9 and en <= 1e-9 and ek <= 1e-9, (tag, ea, en, ek)


def test_scanpath_saliency_and_evaluation_match_the_reference(gold):
    from scanpaths_amd.utils import evaluation as E
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    frame = (240, 320)
    n = 0
    for i, (shape, sigma) in enumerate(zip(gold["e2e/shapes"], gold["e2e/sigmas"])):
        shape = (int(shape[0]), int(shape[1]))
        for j, mode in enumerate(("constant", "reflect")):
            p = f"e2e/{i}/{j}/"
            gt, gt_g = _paths(gold, p + "gt_")
            pr, pr_g = _paths(gold, p + "pred_")
            res = M.scanpath_saliency(gt, gt_g, pr, pr_g, frame, float(sigma), output_shape=shape, mode=mode)
            assert all(res[k].is_cuda and res[k].dtype == torch.float64 and tuple(res[k].shape) == (5,) for k in ("AUC_Judd", "NSS", "KLdiv"))
            _check_scores(f"scanpath_saliency {shape} sigma {sigma} {mode}", res, gold, p)
            assert np.array_equal(res["gt_dropped"].cpu().numpy(), gold[p + "gt_dropped"])
            assert np.array_equal(res["pred_dropped"].cpu().numpy(), gold[p + "pred_dropped"])
            again = M.scanpath_saliency(gt, gt_g, pr, pr_g, frame, float(sigma), output_shape=shape, mode=mode)
            assert all(torch.equal(_bits(res[k]), _bits(again[k])) for k in ("AUC_Judd", "NSS", "KLdiv"))
            # the same through keys: question ids in first-appearance order of the human scanpaths
            names = [f"q{100 - q}" for q in range(5)]
            means, per_key = E.saliency_evaluation(gt, pr, [names[q] for q in gt_g], [names[q] for q in pr_g], frame, sigma=float(sigma),
                                                   output_shape=shape, mode=mode)
            assert per_key["keys"] == names
            _check_scores(f"saliency_evaluation {shape} {mode}", per_key, gold, p)
            for m, ref in (("AUC_Judd", gold[p + "auc"]), ("NSS", gold[p + "nss"]), ("KLdiv", gold[p + "kld"])):
                assert means[m + "_nan"] == int(np.isnan(ref).sum())
                assert abs(means[m] - np.nanmean(ref)) <= 1e-9 * max(1.0, abs(np.nanmean(ref)))
            n += 1
    assert n >= 6
    # keys in another order than the groups, the run_test_loop records as predictions, an unknown key
    p = "e2e/0/0/"
    gt, gt_g = _paths(gold, p + "gt_")
    pr, pr_g = _paths(gold, p + "pred_")
    order = np.argsort([-q for q in gt_g], kind="stable")                      # human scanpaths of question 4 first
    recs = [{"qid": q, "X": list(a[:, 0]), "Y": list(a[:, 1]), "T": list(a[:, 2] * 1000)} for a, q in zip(pr, pr_g)]
    fvs, keys = E.predict_results_fix_vectors(recs)
    means, per_key = E.saliency_evaluation([gt[k] for k in order], fvs, [gt_g[k] for k in order], keys, sigma=1.5, output_shape=(30, 40))
    assert per_key["keys"] == [4, 3, 2, 1, 0]
    back = {k: v[::-1] for k, v in per_key.items() if k != "keys"}
    with np.errstate(all="ignore"):
        # T went through * 1000 / 1000: the count maps do not depend on it
        _check_scores("saliency_evaluation from records", back, gold, p)
    with pytest.raises(ValueError, match="not among gt_keys"):
        E.saliency_evaluation(gt, pr, gt_g, [q + 5 for q in pr_g], sigma=1.5, output_shape=(30, 40))


def test_fixmaps_c_abi_error_codes():
    """unsupported mode -> SP_EINVAL, null buffers -> SP_ENULL: never a crash, never a silent fallback"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    L = hip.lib()
    st = hip.stream()
    x = torch.zeros((2, 8, 8), dtype=torch.float64, device=DEV)
    w = torch.ones(1, dtype=torch.float64, device=DEV)
    ws = torch.zeros(int(L.sp_gaussian_blur_maps_workspace(2, 8, 8)), dtype=torch.uint8, device=DEV)
    assert ws.numel() == 2 * 8 * 8 * 8
    ok = (hip.ptr(x), 2, 8, 8, hip.ptr(w), 0, hip.ptr(w), 0)
    assert L.sp_gaussian_blur_maps(*ok, 0, 0, hip.ptr(ws), hip.ptr(x), st) == 0
    for mode in (3, -1, 7):                                                    # wrap / mirror / anything else
        assert L.sp_gaussian_blur_maps(*ok, mode, 0, hip.ptr(ws), hip.ptr(x), st) == -1
    assert L.sp_gaussian_blur_maps(*ok, 0, 3, hip.ptr(ws), hip.ptr(x), st) == -1              # normalisation
    assert L.sp_gaussian_blur_maps(hip.ptr(x), 2, 8, 8, hip.ptr(w), -1, hip.ptr(w), 0, 0, 0, hip.ptr(ws), hip.ptr(x), st) == -1
    big = L.sp_gaussian_blur_maps_max_axis() + 1
    assert big > 320
    assert L.sp_gaussian_blur_maps(hip.ptr(x), 1, big, 1, hip.ptr(w), 0, hip.ptr(w), 0, 0, 0, hip.ptr(ws), hip.ptr(x), st) == -1
    assert L.sp_gaussian_blur_maps(None, 2, 8, 8, hip.ptr(w), 0, hip.ptr(w), 0, 0, 0, hip.ptr(ws), hip.ptr(x), st) == -2
    assert L.sp_gaussian_blur_maps(hip.ptr(x), 2, 8, 8, None, 0, hip.ptr(w), 0, 0, 0, hip.ptr(ws), hip.ptr(x), st) == -2
    assert L.sp_gaussian_blur_maps(*ok, 0, 0, None, hip.ptr(x), st) == -2
    assert L.sp_gaussian_blur_maps(*ok, 0, 0, hip.ptr(ws), None, st) == -2
    fix = torch.zeros((4, 3), dtype=torch.float64, device=DEV)
    start = torch.zeros(1, dtype=torch.int64, device=DEV)
    cnt = torch.full((1,), 4, dtype=torch.int32, device=DEV)
    grp = torch.zeros(1, dtype=torch.int32, device=DEV)
    drop = torch.zeros(2, dtype=torch.int32, device=DEV)
    args = (hip.ptr(fix), 3, hip.ptr(start), hip.ptr(cnt), hip.ptr(grp), 1, 2, 8, 8, 8.0, 8.0)
    assert L.sp_fixation_maps(*args, 1, hip.ptr(x), hip.ptr(drop), st) == 0
    assert float(x[0, 0, 0]) == 4.0 and float(x.sum()) == 4.0
    assert L.sp_fixation_maps(*args, 3, hip.ptr(x), hip.ptr(drop), st) == -1                    # weight
    assert L.sp_fixation_maps(hip.ptr(fix), 2, hip.ptr(start), hip.ptr(cnt), hip.ptr(grp), 1, 2, 8, 8, 8.0, 8.0, 2, hip.ptr(x), hip.ptr(drop),
                              st) == -1                                                         # duration sum without a duration column
    assert L.sp_fixation_maps(hip.ptr(fix), 3, hip.ptr(start), hip.ptr(cnt), hip.ptr(grp), 1, 2, 8, 8, 0.0, 8.0, 0, hip.ptr(x), hip.ptr(drop),
                              st) == -1                                                         # empty frame
    assert L.sp_fixation_maps(*args, 0, None, hip.ptr(drop), st) == -2
    assert L.sp_fixation_maps(*args, 0, hip.ptr(x), None, st) == -2
    assert L.sp_fixation_maps(None, 3, hip.ptr(start), hip.ptr(cnt), hip.ptr(grp), 1, 2, 8, 8, 8.0, 8.0, 0, hip.ptr(x), hip.ptr(drop), st) == -2
    out = torch.zeros(2, dtype=torch.int32, device=DEV)
    assert L.sp_count_positive(hip.ptr(x), 2, 64, hip.ptr(out), st) == 0 and out.tolist() == [1, 0]
    assert L.sp_count_positive(None, 2, 64, hip.ptr(out), st) == -2 and L.sp_count_positive(hip.ptr(x), 0, 64, hip.ptr(out), st) == -1
    with pytest.raises(ValueError):
        M.density_maps(x, 2.0, mode="wrap")
    with pytest.raises(ValueError):
        M.density_maps(torch.zeros((1, big, 2), dtype=torch.float64, device=DEV), 2.0)
    with pytest.raises(hip.HipError):
        hip.check(L.sp_gaussian_blur_maps(*ok, 5, 0, hip.ptr(ws), hip.ptr(x), st), "sp_gaussian_blur_maps")
