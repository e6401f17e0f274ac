"""csrc/scankde.hip through evaltools.scanpath_kde, the keyed evaluation and the loop, against the restatement
tests/scanpath_kde_ref.py on the shared inputs of tests/scanpath_kde_cases.py.

The bar.  n, others, dropped, the NaN / -inf pattern of every output and the "best" bandwidth must be EQUAL.  Log-valued outputs must
stay within 1e-12 * max(1, |ref|), table cells within 1e-12 of the all-image total of their cell: the restatement's quick form sums
pairwise, the device serially, and the two exp / log2 implementations may differ in the last bit -- the bar of §15 and §19, for their
reasons.  On these inputs a serial and a lane-strided-plus-butterfly summation of the same kernel values differ by 1.9e-15 of
max(1, |bits|) (tests/test_scanpath_kde_cpu.py prints it), the plain loops and the quick form by 1.9e-15: the bar leaves a factor of
about 500.  Every test prints its worst error; measured on an MI355X: leave="image" 5.1e-15, "scanpath" 9.6e-16,
"scanpath_step" 1.3e-15, search means 2.1e-15, table cells 8.4e-16 of the cell's total, against LL - IG of sp_scan_likelihood 1.3e-15.

Runs per map: uniform_mix 0.01 with all five bandwidths (1e-3, 0.5, one cell pitch, 45.3, 1e6) and every fixation; uniform_mix 0 with
1e-3, 45.3 and 1e6 and max_length 4 -- the bandwidths at which no exponent argument of these inputs lies between -800 and -700 (asserted
on the restatement), so that underflow to an exact zero, and with it every -inf, is unambiguous; on the 3 x 5 map also uniform_mix 0.5
with max_length 16, and max_length 1."""
import numpy as np
import pytest
import torch

import scanpath_kde_cases as C
import scanpath_kde_ref as R

pytestmark = pytest.mark.gpu
TOL = 1e-12
_REF = {}


def M():
    from scanpaths_amd.utils.evaltools import scanpath_kde
    return scanpath_kde


def quick(shape, max_length=None, big=None):
    """the restatement's arrays of a case, built once"""
    key = (shape, max_length, big)
    if key not in _REF:
        paths, groups, frame = C.case(shape, big)
        _REF[key] = R.Quick(paths, groups, frame, shape, max_length)
    return _REF[key]


def compare(got, ref, what):
    """the exact parts equal, the finite values within the bar -> the worst error in units of max(1, |ref|)"""
    for k in ("n", "others", "dropped"):
        assert got[k].dtype == np.int32 and got[k].shape == ref[k].shape and (got[k] == ref[k]).all(), (what, k)
    a, b = got["LL"], ref["LL"]
    assert a.dtype == np.float64 and a.shape == b.shape, what
    assert (np.isnan(a) == np.isnan(b)).all() and (np.isneginf(a) == np.isneginf(b)).all() and not np.isposinf(a).any(), what
    fin = np.isfinite(b)
    err = float((np.abs(a[fin] - b[fin]) / np.maximum(1.0, np.abs(b[fin]))).max()) if fin.any() else 0.0
    assert err <= TOL, (what, err)
    return err


def device_all(shape, bws, u, leave, max_length, big=None):
    """all bandwidths in ONE call (the layer under the three public calls) -> one public-format dict per bandwidth"""
    paths, groups, frame = C.case(shape, big)
    p, LL, others, valid = M()._leave_out(paths, groups, frame, shape, bws, u, leave, max_length)
    assert LL.shape == (p.N, len(bws))
    return [dict(LL=p.scatter(LL[:, k], np.nan, np.float64), others=p.scatter(others, 0, np.int32), n=p.n,
                 dropped=np.bincount(p.path[valid == 0], minlength=p.S).astype(np.int32)) for k in range(len(bws))]


RUNS = [(shape, 0.01, None) for shape in C.MAPS] + [(shape, 0.0, 4) for shape in C.MAPS] + [((3, 5), 0.5, 16), ((3, 5), 0.01, 1)]


@pytest.mark.parametrize("shape,u,max_length", RUNS, ids=lambda v: str(v).replace(" ", ""))
def test_leave_out_scores(shape, u, max_length):
    bws = list(C.BW0) if u == 0.0 else C.bandwidths(shape)
    q = quick(shape, max_length)
    if u == 0.0:                                                 # the condition on the inputs, on the restatement alone
        for b in bws:
            args = q.exponent_args(b)
            assert ((args > -700.0) | (args < -800.0)).all(), (shape, b)
    worst, ninf = {}, 0
    for leave in R.LEAVE:
        got = device_all(shape, bws, u, leave, max_length)
        for b, g in zip(bws, got):
            ref = q.leave_out(b, u, leave)
            worst[leave] = max(worst.get(leave, 0.0), compare(g, ref, (shape, u, max_length, leave, b)))
            ninf += int(np.isneginf(ref["LL"]).sum())
            if shape == (1, 1):
                assert (g["LL"][~np.isnan(g["LL"])] == 0.0).all() or u > 0.0      # P = 1: every score is 0 (up to (1 - u) + u)
                assert np.abs(g["LL"][~np.isnan(g["LL"])]).max() <= 2e-16
    one = np.array(C.case(shape)[1]) == C.IDS["one"]             # the image with one scanpath has no other scanpath
    assert (got[0]["others"][one] == 0).all() and np.isnan(got[0]["LL"][one]).all()
    print(f"KDE leave-out {shape} u={u} max_length={max_length}: worst error " + ", ".join(f"{k} {v:.1e}" for k, v in worst.items())
          + f"; -inf scores {ninf}")
    assert u > 0.0 or shape == (1, 1) or ninf > 0                # the u = 0 runs do meet exact zeros


def test_public_calls_and_bandwidth_search():
    shape = (30, 40)
    paths, groups, frame = C.case(shape, big=False)
    res = M().kde_leave_out_likelihood(paths, groups, frame, shape, bandwidth=16.0, uniform_mix=0.01, leave="scanpath_step", max_length=16)
    assert list(res) == ["LL", "others", "n", "dropped"] and res["LL"].shape == (len(paths), 16)
    compare(res, quick(shape, 16, False).leave_out(16.0, 0.01, "scanpath_step"), "public")
    worst = 0.0
    for leave, bws in (("image", [45.3]), ("scanpath", 2.0 ** np.arange(2.0, 7.01, 1 / 3)), ("scanpath_step", [4.0, 16.0, 64.0])):
        assert len(bws) in (1, 3, M().MAX_BANDWIDTHS)            # K = 1 and K = the limit
        got = M().kde_bandwidth_search(paths, groups, frame, shape, bandwidths=bws, uniform_mix=0.01, leave=leave)
        ref = R.search(paths, groups, frame, shape, list(bws), 0.01, leave)
        top = np.sort(ref["LL"])[::-1]
        assert len(top) == 1 or top[0] - top[1] > 1e-9           # the condition on the inputs: the best mean is not a near tie
        assert list(got) == ["bandwidths", "LL", "sum", "count", "best"] and (got["bandwidths"] == ref["bandwidths"]).all()
        assert got["count"] == ref["count"] > 0 and got["best"] == ref["best"]
        for k in ("LL", "sum"):
            err = float((np.abs(got[k] - ref[k]) / np.maximum(1.0, np.abs(ref[k]))).max())
            assert err <= TOL, (leave, k, err)
            worst = max(worst, err)
        if len(bws) > 3:
            assert bws[0] < got["best"] < bws[-1]                # an interior maximum
    print(f"KDE bandwidth search: worst error of the means and sums {worst:.1e}")
    with pytest.raises(ValueError, match="kernel limit"):
        M().kde_leave_out_likelihood(paths, groups, frame, (1, 2049), bandwidth=16.0, uniform_mix=0.01, leave="image")


@pytest.mark.parametrize("shape", list(C.MAPS), ids=str)
def test_cell_baselines(shape):
    from scanpaths_amd.utils.evaltools.scanpath_likelihood import cell_baselines
    paths, groups, frame = C.case(shape, big=False)
    P, worst = shape[0] * shape[1], 0.0
    for b, ml in zip(C.bandwidths(shape), (None, 1, 4, 16, None)):
        q = quick(shape, ml, False)
        got = M().kde_cell_baselines(paths, groups, frame, shape, bandwidth=b, max_length=ml)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (max(groups) + 1, P)
        got, ref = got.cpu().numpy(), q.baselines(b)
        total = q.own_tables(b).sum(0).reshape(-1)               # the all-image total of every cell
        err = float((np.abs(got - ref) / np.maximum(total, 1e-300)[None]).max()) if total.max() > 0 else 0.0
        assert (got >= 0.0).all() and err <= TOL, (shape, b, err)
        count = np.bincount(q.g[q.ok], minlength=q.G)
        assert np.abs(got.sum(1) - (count.sum() - count)).max() <= TOL * max(1, count.sum())
        worst = max(worst, err)
    print(f"KDE cell baselines {shape}: worst error {worst:.1e} of the cell's total")
    # without the border fixations of image 3 (between two centres), bandwidth 1e-3 is exactly the histogram of cell_baselines
    keep = [i for i, g in enumerate(groups) if g != C.IDS["two"]]
    sub, subg = [paths[i] for i in keep], [groups[i] for i in keep]
    assert torch.equal(M().kde_cell_baselines(sub, subg, frame, shape, bandwidth=1e-3), cell_baselines(sub, subg, frame, shape))
    # one image: the row is exactly zero; leave="image" has nobody to ask
    mine = [p for p, g in zip(paths, groups) if g == C.IDS["n63"]]
    assert (M().kde_cell_baselines(mine, [0] * 3, frame, shape, bandwidth=C.bandwidths(shape)[2]) == 0.0).all()
    res = M().kde_leave_out_likelihood(mine, [0] * 3, frame, shape, bandwidth=8.0, uniform_mix=0.01, leave="image")
    assert np.isnan(res["LL"]).all() and (res["others"] == 0).all() and res["n"].tolist() == [len(p) for p in mine]


def test_image_score_is_ll_minus_ig_of_the_likelihood_kernel():
    from scanpaths_amd.utils.evaltools.scanpath_likelihood import scanpath_likelihood
    shape, T, u = (30, 40), 16, 0.01
    paths, groups, frame = C.case(shape, big=False)
    keep = [i for i, p in enumerate(paths) if len(p) <= 64]
    paths, groups = [paths[i] for i in keep], [groups[i] for i in keep]
    worst = 0.0
    for b in (0.5, 8.0, 45.3):
        base = M().kde_cell_baselines(paths, groups, frame, shape, bandwidth=b, max_length=T)
        probs = torch.full((1, T, 1 + shape[0] * shape[1]), 1.0 / 1201, device="cuda")
        lik = scanpath_likelihood(probs, paths, [0] * len(paths), frame, uniform_mix=u, metrics=("LL", "IG"), map_shape=shape,
                                  baseline=base, baseline_rows=groups)
        kde = M().kde_leave_out_likelihood(paths, groups, frame, shape, bandwidth=b, uniform_mix=u, leave="image", max_length=T)
        want, got = lik["LL"] - lik["IG"], kde["LL"]
        assert (np.isnan(want) == np.isnan(got)).all() and (kde["n"] == lik["n"]).all() and (kde["dropped"] == lik["dropped"]).all()
        fin = ~np.isnan(want)
        worst = max(worst, float((np.abs(got[fin] - want[fin]) / np.maximum(1.0, np.abs(want[fin]))).max()))
    print(f"KDE leave-image score against LL - IG of sp_scan_likelihood: worst error {worst:.1e}")
    assert worst <= TOL


def test_bit_identical_repeats_and_subsets():
    shape = (30, 40)
    paths, groups, frame = C.case(shape)
    kw = dict(bandwidth=11.3, uniform_mix=0.0)
    for leave in ("scanpath", "scanpath_step"):
        full = M().kde_leave_out_likelihood(paths, groups, frame, shape, leave=leave, **kw)
        again = M().kde_leave_out_likelihood(paths, groups, frame, shape, leave=leave, **kw)
        assert full["LL"].tobytes() == again["LL"].tobytes()
        # the gold standard of two of the images alone, under other ids and in another order of the images
        keep = [i for i, g in enumerate(groups) if g in (C.IDS["many"], C.IDS["two"])]
        sub = M().kde_leave_out_likelihood([paths[i] for i in keep], [40 - groups[i] for i in keep], frame, shape, leave=leave, **kw)
        assert sub["LL"].tobytes() == full["LL"][keep][:, :sub["LL"].shape[1]].tobytes() and not np.isnan(sub["LL"]).all()
        assert (sub["others"] == full["others"][keep]).all()
    a = M().kde_leave_out_likelihood(paths, groups, frame, shape, leave="image", **kw)
    b = M().kde_leave_out_likelihood(paths, groups, frame, shape, leave="image", **kw)
    assert a["LL"].tobytes() == b["LL"].tobytes()
    t1 = M().kde_cell_baselines(paths, groups, frame, shape, bandwidth=11.3)
    assert torch.equal(t1, M().kde_cell_baselines(paths, groups, frame, shape, bandwidth=11.3))


def test_keyed_evaluation_table_and_loop(monkeypatch):
    from scanpaths_amd import inference
    from scanpaths_amd.utils import evaluation as E
    shape, frame, T, u, b = (30, 40), (240, 320), 4, 0.01, 20.0
    g = np.random.default_rng(5)

    def fv(n):
        return np.stack([g.uniform(0, 320, n), g.uniform(0, 240, n), g.uniform(0.1, 0.5, n)], 1)

    fix_vectors = [[fv(3), fv(6), fv(4)], [fv(5)], [fv(2), fv(7)], [fv(4), fv(4), fv(1), fv(0)]]
    fix_vectors[0][1][1, 0] = 400.0                                                   # a dropped fixation
    keys = ["q1", "q2", "q1", "q3"]                                                   # a key on two samples; a sample with one subject
    flat = [p for s in fix_vectors for p in s]
    sample = np.repeat(np.arange(4), [len(s) for s in fix_vectors])
    for same_step, leave in ((False, "scanpath"), (True, "scanpath_step")):
        ref = R.leave_out(flat, sample, frame, shape, b, u, leave, T)                 # the plain loops
        means, per_key = E.likelihood_gold_standard_evaluation(fix_vectors, keys, bandwidth=b, uniform_mix=u, max_length=T,
                                                               same_step=same_step)
        total, count = R.pooled(ref["LL"])
        assert means["GOLD_count"] == count > 0 and abs(means["GOLD"] - total / count) <= TOL * max(1.0, abs(total / count))
        assert means["dropped"] == 1 and means["GOLD_nan"] == int(np.isnan(ref["LL"]).sum() - (np.arange(ref["LL"].shape[1])[None]
                                                                                                >= ref["n"][:, None]).sum())
        assert per_key["keys"] == ["q1", "q2", "q3"] and np.isnan(per_key["GOLD"][1]) and means["GOLD_nan_keys"] == 1
        q1 = ref["LL"][np.isin(sample, (0, 2))]
        assert abs(per_key["GOLD"][0] - np.nanmean(q1)) <= TOL * max(1.0, abs(np.nanmean(q1))) and per_key["dropped"].tolist() == [1, 0, 0]
    probs = torch.rand(4, T, 1201, generator=torch.Generator().manual_seed(3)) + 0.01

    class Stub:
        calls = 0

        def eval(self):
            return self

        def __call__(self, images, attention_maps):
            lo = 2 * (Stub.calls % 2)
            Stub.calls += 1
            return {"all_actions_prob": probs[lo:lo + 2].cuda()}

    loader = [{"images": torch.zeros(2, 3, 8, 8), "attention_maps": torch.zeros(2, 1, 8, 8), "fix_vectors": fix_vectors[lo:lo + 2],
               "question_ids": keys[lo:lo + 2]} for lo in (0, 2)]
    plain, plain_keys = inference.run_likelihood_loop(Stub(), loader, uniform_mix=u, metrics=("LL", "NSS"))
    none, none_keys = inference.run_likelihood_gold_loop(Stub(), loader, gold_standard=None, uniform_mix=u, metrics=("LL", "NSS"))
    assert set(none) == set(plain) and all(none[k] == plain[k] or (np.isnan(none[k]) and np.isnan(plain[k])) for k in plain)
    gold = dict(bandwidth=b, uniform_mix=u, max_length=T, same_step=True)
    both, both_keys = inference.run_likelihood_gold_loop(Stub(), loader, gold_standard=gold, uniform_mix=u, metrics=("LL", "NSS"))
    assert all(both[k] == plain[k] or (np.isnan(both[k]) and np.isnan(plain[k])) for k in plain)      # today's table, and more
    assert set(both) - set(plain) == {"GOLD", "GOLD_sum", "GOLD_count", "GOLD_nan", "GOLD_nan_keys"}
    assert both["GOLD_count"] == means["GOLD_count"] and abs(both["GOLD"] - means["GOLD"]) <= TOL * max(1.0, abs(means["GOLD"]))
    assert [list(k) for k in both_keys] == [list(k) + ["GOLD"] for k in plain_keys] and len(both_keys[0]["GOLD"]) == 2
    res = E.information_gain_explained(both, both)
    assert np.isnan(res["IGE"]) and res["GOLD_count"] == both["GOLD_count"] and res["IG_count"] == 0   # no IG was asked for
