"""The model's fixation density in closed form on the device against the plain-loop restatement
tests/expected_maps_ref.py: maps, fixations and bad bit for bit (NaN equal to NaN) through the C entry point and through
expected_fixation_maps; the cell-pixel table against the sampler's own kernel; the closed form against the sampler's and the
rasteriser's kernels over all action sequences; the scoring path with prediction="maps"; the keyed call, the table, the loop."""
import itertools
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import expected_maps_ref as X
from helpers import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
MAPS = {(1, 1): (75, 100), (2, 3): (20, 45), (5, 7): (100, 300), (30, 40): (240, 320), (32, 64): (256, 512)}   # (5, 7): cells that are not square
OUTPUTS = (None, (7, 11), (2, 2))               # the frame (more pixels than cells: empty pixels), no divisor of anything, cells that share pixels
ALL = ("sAUC", "CC", "SIM", "IG")
_CASES = {}


def S():
    from scanpaths_amd.utils.evaltools import saliency_maps
    return saliency_maps


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def same(got, want, what):
    got = got.cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    bad = np.flatnonzero(~((got == want) | (np.isnan(got) & np.isnan(want))).reshape(-1)) if got.dtype.kind == "f" \
        else np.flatnonzero((got != want).reshape(-1))
    assert not len(bad), (what, len(bad), bad[:5], got.reshape(-1)[bad[:5]], want.reshape(-1)[bad[:5]])


def case(shape, T):
    """raw positive float32 rows, not normalised: 0 good, 1 a zero-mass step at t = min(1, T - 1), 2 good, 3 good, 4 an inf cell at
    t = 0, 5 good (the C entry point gives it a group that does not exist); weights in (0, 3) with a NaN for row 3 at the LAST step (bad
    only when that step counts) and a negative one for row 5 at t = 0; per-row references are cached per (min_length, Tm, weighted)"""
    key = (shape, T)
    if key not in _CASES:
        P = shape[0] * shape[1]
        g = np.random.default_rng(100 * P + T)
        probs = g.uniform(0.01, 1.0, (6, T, 1 + P)).astype(np.float32)
        probs[1, min(1, T - 1), :] = 0.0
        probs[4, 0, 1 + P // 2] = float("inf")
        weight = g.uniform(0.0, 3.0, (6, T))
        weight[3, T - 1], weight[5, 0] = float("nan"), -1.0
        _CASES[key] = (probs, weight, {})
    return _CASES[key]


def combos(T):
    """(min_length, max_steps): min_length 0, 2, T + 1 and max_steps 1, 2, T, 64"""
    return sorted({(0, 1), (2, 2), (T + 1, T), (0, 64), (2, T), (T + 1, 64)})


def reference(shape, T, rows, groups, G, min_length, max_steps, out, weighted):
    probs, weight, cache = case(shape, T)
    per_row = cache.setdefault((min_length, min(T, max_steps), weighted), [None] * 6)
    frame = MAPS[shape]
    H, W = frame if out is None else out
    sub = [per_row[r] for r in rows]
    res = X.expected_fixation_maps(probs[rows], weight[rows] if weighted else None, groups, G, min_length, max_steps,
                                   X_TABLE(shape, out), H, W, rows=sub)
    for r, v in zip(rows, res["rows"]):
        per_row[r] = v
    return res


def X_TABLE(shape, out):
    """the package's table (from the sampler's kernel): the restatement is handed the same one, it is checked on its own below"""
    return S().expected_cell_pixels(shape, MAPS[shape], out)


def call_c(probs, weight, groups, G, min_length, max_steps, table, H, W):
    """the C entry point itself, on poisoned maps and scratch: a NaN that survives shows an element nobody wrote, or a read of scratch
    nobody wrote"""
    from scanpaths_amd import hip
    from scanpaths_amd.utils.evaltools import _batch
    L = hip.model_lib()
    R, T, A = probs.shape
    sections = dict(row_group=np.asarray(groups, np.int32), cell_pixel=np.asarray(table, np.int32))
    if weight is not None:
        sections["step_weight"] = np.ascontiguousarray(weight, np.float64)
    buf, at = _batch.upload(sections, dev())
    p = torch.from_numpy(probs).to(dev())
    n = L.sp_model_fixation_expectation_workspace(R, T, shape_of(A, table)[0], shape_of(A, table)[1], G, max_steps)
    work = torch.full((int(n),), float("nan"), dtype=torch.float64, device=dev())
    maps = torch.full((G, H, W), float("nan"), dtype=torch.float64, device=dev())
    out = _batch.Out({"fixations": (np.float64, R), "bad": (np.int32, R)}, dev())
    Hm, Wm = shape_of(A, table)
    hip.check(L.sp_model_fixation_expectation(hip.ptr(p), at.get("step_weight"), at["row_group"], R, T, Hm, Wm, G, min_length, max_steps,
                                              at["cell_pixel"], H, W, hip.ptr(work), hip.ptr(maps), out.ptr("fixations"), out.ptr("bad"),
                                              hip.stream()), "sp_model_fixation_expectation")
    return dict(out.host(), maps=maps.cpu().numpy())


_SHAPE = {1 + h * w: (h, w) for h, w in MAPS}


def shape_of(A, table):
    return _SHAPE[A]


# ---- restatement parity --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 2, 3, 16])
@pytest.mark.parametrize("shape", list(MAPS))
def test_c_entry_point_equals_the_restatement_bit_for_bit(shape, T):
    probs, weight, _ = case(shape, T)
    rows = [0, 1, 2, 3, 4, 5]
    G = 4                                                                # group 1 stays empty, group 3 holds only the zero-mass row
    for n, (min_length, max_steps) in enumerate(combos(T)):
        out = OUTPUTS[n % len(OUTPUTS)]
        H, W = MAPS[shape] if out is None else out
        table = X_TABLE(shape, out)
        groups = [0, 3, 2, 0, 2, -1 if n % 2 else G]                     # interleaved; row 5: a group that does not exist
        want = reference(shape, T, rows, groups, G, min_length, max_steps, out, False)
        got = call_c(probs, None, groups, G, min_length, max_steps, table, H, W)
        what = (shape, T, min_length, max_steps, out)
        for k in ("maps", "fixations", "bad"):
            same(got[k], want[k], (k,) + what)
        zero = 1 if min(1, T - 1) < min(T, max_steps) else 0             # the zero-mass step counts unless max_steps cuts it off
        assert got["bad"].tolist() == [0, zero, 0, 0, 1, -1] and np.isnan(got["fixations"][[4, 5]]).all()
        assert not got["maps"][1].any() and got["maps"][3].any() == (zero == 0) and got["maps"][0].any()
        ones = call_c(probs, np.ones((6, T)), groups, G, min_length, max_steps, table, H, W)      # NULL against all-ones: identical bits
        for k in ("maps", "fixations", "bad"):
            same(ones[k], got[k], (k, "ones") + what)
        wantw = reference(shape, T, rows, [0, 3, 2, 0, 2, 1], G, min_length, max_steps, out, True)
        gotw = call_c(probs, weight, [0, 3, 2, 0, 2, 1], G, min_length, max_steps, table, H, W)
        for k in ("maps", "fixations", "bad"):
            same(gotw[k], wantw[k], (k, "weighted") + what)
        # the NaN weight sits at the last step: bad only when that step counts; the negative weight at t = 0 always is
        assert gotw["bad"].tolist() == [0, zero, 0, 1 if max_steps >= T else 0, 1, 1] and not gotw["maps"][1].any()
    if shape != (1, 1):
        wild = np.array(X_TABLE(shape, None))                           # a table the Python layer never passes: entries outside [0, H W)
        wild[0], wild[-1] = -1, MAPS[shape][0] * MAPS[shape][1]
        H, W = MAPS[shape]
        got = call_c(probs[:3], None, [0, 0, 0], 1, 0, 64, wild, H, W)
        want = X.expected_fixation_maps(probs[:3], None, [0, 0, 0], 1, 0, 64, wild, H, W)
        same(got["maps"], want["maps"], ("skipped cells", shape, T))


@pytest.mark.parametrize("T", [1, 2, 3, 16])
@pytest.mark.parametrize("shape", list(MAPS))
def test_python_layer_equals_the_restatement_bit_for_bit(shape, T):
    probs, weight, _ = case(shape, T)
    frame = MAPS[shape]
    finite = np.where(np.isfinite(weight) & (weight >= 0), weight, 0.5)
    dp = torch.from_numpy(probs).to(dev())
    for n, (min_length, max_steps) in enumerate(combos(T)):
        out = OUTPUTS[(n + 1) % len(OUTPUTS)]
        H, W = frame if out is None else out
        for rows, groups, G in (([0], [0], 1), ([0, 2, 3], [1, 0, 1], 2), ([0, 1, 2, 3, 4], [0, 3, 2, 0, 2], 4)):       # R = 1, 3, 5
            want = reference(shape, T, rows, groups, G, min_length, max_steps, out, False)
            got = S().expected_fixation_maps(dp[rows], groups, G, min_length=min_length, max_steps=max_steps, frame_size=frame,
                                             output_shape=out, map_shape=shape)
            assert set(got) == {"maps", "fixations", "bad"} and got["maps"].is_cuda and tuple(got["maps"].shape) == (G, H, W)
            for k in ("maps", "fixations", "bad"):
                same(got[k], want[k], (k, shape, T, min_length, max_steps, out, rows))
        rows, groups = [0, 2, 3, 5], [1, 0, 1, 0]
        wantw = X.expected_fixation_maps(probs[rows], finite[rows], groups, 2, min_length, max_steps, X_TABLE(shape, out), H, W)
        for sw in (finite[rows], torch.from_numpy(finite[rows]).to(dev())):
            gotw = S().expected_fixation_maps(dp[rows].double(), groups, 2, min_length=min_length, max_steps=max_steps, frame_size=frame,
                                              output_shape=out, map_shape=shape, step_weight=sw)
            for k in ("maps", "fixations", "bad"):
                same(gotw[k], wantw[k], (k, "weighted", shape, T, min_length, max_steps, out))
    if shape == (30, 40):                                                # 1201 actions: the one default map shape
        got = S().expected_fixation_maps(dp[[0]], [0], 1, min_length=1, max_steps=64, frame_size=frame)
        same(got["maps"], reference(shape, T, [0], [0], 1, 1, 64, None, False)["maps"], "default map shape")
        total = float(got["maps"].sum())
        assert abs(total - got["fixations"][0]) <= 64 * 2.0 ** -53 * 1201 * total                   # the map holds the expected fixations
    else:
        with pytest.raises(ValueError, match="map_shape is required"):
            S().expected_fixation_maps(dp[[0]], [0], 1, min_length=1, max_steps=64, frame_size=frame)


# ---- the cell-pixel table against the sampler's own kernel --------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(MAPS))
def test_cell_pixel_table_is_where_the_samplers_fixation_lands(shape):
    """all P actions go through Sampling.generate_scanpath and fixation_maps(.., "count"), one map per action (256 at a time): the one
    counted pixel of action k is table[k - 1], for every output shape"""
    from scanpaths_amd.models.sampling import Sampling
    Hm, Wm = shape
    fh, fw = MAPS[shape]
    P = Hm * Wm
    s = Sampling(convLSTM_length=1, min_length=0, map_width=Wm, map_height=Hm, width=fw, height=fh)
    acts = torch.arange(1, P + 1, dtype=torch.int64, device=dev()).reshape(P, 1)
    fvs, _, _ = s.generate_scanpath(torch.zeros(1), None, torch.ones(P, 1, device=dev()), acts)
    paths = [np.stack([fv["start_x"], fv["start_y"]], 1) for fv in fvs]
    assert all(len(p) == 1 for p in paths)
    for out in OUTPUTS + ((3 * Hm, 2 * Wm),):
        table = S().expected_cell_pixels(shape, (fh, fw), out)
        assert table.dtype == np.int32 and table.shape == (P,) and not table.flags.writeable
        assert S().expected_cell_pixels(shape, (fh, fw), out) is table                       # cached
        H, W = (fh, fw) if out is None else out
        assert table.min() >= 0 and table.max() < H * W
        for lo in range(0, P, 256):
            hi = min(P, lo + 256)
            maps, dropped = S().fixation_maps(paths[lo:hi], np.arange(hi - lo), (fh, fw), out, "count", num_groups=hi - lo)
            flat = maps.reshape(hi - lo, -1)
            assert not dropped.any() and bool((flat.sum(1) == 1.0).all()) and bool((flat.max(1).values == 1.0).all())
            assert np.array_equal(flat.argmax(1).cpu().numpy(), table[lo:hi]), (shape, out, lo)
        if shape == (30, 40):
            assert np.array_equal(table, X.cell_pixels(shape, (fh, fw), out)), out             # the float32 restatement, exactly
        else:
            print(shape, out, "cells where the float32 restatement differs:", int((table != X.cell_pixels(shape, (fh, fw), out)).sum()))
    if shape == (5, 7):
        assert (np.bincount(S().expected_cell_pixels(shape, (fh, fw), (2, 2)), minlength=4) > 1).all()     # every list longer than one


# ---- the closed form against the sampler's and the rasteriser's kernels, over all sequences ----------------------------------------------
def test_sampled_and_exact_maps_agree_over_all_sequences():
    """all 5^3 action sequences of a T = 3, 2 x 2 case on 75 x 100 go through Sampling.generate_scanpath and fixation_maps (one map per
    sequence), weight "count" and -- with the step's fixed float32 durations on both sides -- "duration"; weighted by their exact
    probabilities they give expected_fixation_maps within expected_maps_ref.bound (derived from the operation counts there: the
    enumeration's 5^3 terms per entry plus the closed form's own roundings, p_0 / Z <= 20 for these inputs)"""
    from scanpaths_amd.models.sampling import Sampling
    T, Hm, Wm = 3, 2, 2
    frame = (75, 100)
    g = np.random.default_rng(31)
    probs = g.uniform(0.05, 1.0, (2, T, 5)).astype(np.float32)
    assert (probs[:, :, 0] / probs[:, :, 1:].sum(2)).max() <= 20.0
    step_duration = np.array([0.25, 0.1, 0.7], dtype=np.float32)         # 0.1f and 0.7f are not dyadic-short: the sums must be carried exactly
    seqs = np.array(list(itertools.product(range(5), repeat=T)), dtype=np.int64)
    durations = torch.from_numpy(np.tile(step_duration, (len(seqs), 1))).to(dev())
    for min_length in (0, 1):
        s = Sampling(convLSTM_length=T, min_length=min_length, map_width=Wm, map_height=Hm, width=100, height=75)
        fvs, _, _ = s.generate_scanpath(torch.zeros(1), None, durations, torch.from_numpy(seqs).to(dev()))
        paths = [np.stack([fv["start_x"], fv["start_y"], fv["duration"]], 1) for fv in fvs]
        weights = []
        for row in range(2):
            step = X.step_distributions(probs[row], min_length)
            weights.append([step[0][a] * step[1][b] * step[2][c] for a, b, c in seqs])
            assert sum(weights[-1]) == 1
        for out, kind in itertools.product((None, (1, 2), (3, 5)), ("count", "duration")):
            H, W = frame if out is None else out
            maps, dropped = S().fixation_maps(paths, np.arange(len(seqs)), frame, out, kind, num_groups=len(seqs))
            maps = maps.cpu().numpy().reshape(len(seqs), H * W)
            assert not dropped.any()
            sw = None if kind == "count" else np.tile(step_duration.astype(np.float64), (2, 1))
            exact = S().expected_fixation_maps(torch.from_numpy(probs).to(dev()), [0, 1], 2, min_length=min_length, max_steps=T,
                                               frame_size=frame, output_shape=out, map_shape=(Hm, Wm), step_weight=sw)
            table = S().expected_cell_pixels((Hm, Wm), frame, out)
            bound = X.bound(4, T, int(np.bincount(table).max()), 20.0)
            got = exact["maps"].cpu().numpy().reshape(2, H * W)
            used = np.flatnonzero(maps.any(0))
            assert set(used) == set(table.tolist()) and not np.delete(got, used, 1).any()          # a pixel without a cell is exactly 0
            for row in range(2):
                for px in used:
                    want = float(sum(w * Fraction(float(maps[k, px])) for k, w in enumerate(weights[row]) if maps[k, px]))
                    assert abs(want - got[row, px]) <= bound * want, (min_length, out, kind, row, px, want, got[row, px], bound)
                if kind == "count":
                    n = float(sum(w * len(list(itertools.takewhile(lambda a: a != 0, seq))) for seq, w in zip(seqs, weights[row])))
                    assert abs(n - exact["fixations"][row]) <= bound * n


# ---- the scoring path ---------------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int64) if t.dtype == torch.float64 else t.detach().cpu()


def _golden_cases():
    """the end-to-end cases of tests/golden/fixmaps.npz, the fixtures of tests/test_fixmaps_gpu.py and tests/test_saliency_ext_gpu.py"""
    gold = load_npz(os.path.join(GOLDEN, "fixmaps.npz"))

    def paths(prefix):
        fix, lens = gold[prefix + "fix"], gold[prefix + "len"]
        off = np.concatenate([[0], np.cumsum(lens)])
        return [fix[off[k]:off[k + 1]] for k in range(len(lens))], [int(v) for v in gold[prefix + "group"]]

    for i, (shape, sigma) in enumerate(zip(gold["e2e/shapes"], gold["e2e/sigmas"])):
        for j, mode in enumerate(("constant", "reflect")):
            p = f"e2e/{i}/{j}/"
            yield p, paths(p + "gt_"), paths(p + "pred_"), (int(shape[0]), int(shape[1])), float(sigma), mode, gold


EXTRA = dict(extra_metrics=ALL, uniform_mix=0.01, image_groups=[0, 1, 0, 1, 2])


def test_given_maps_score_bit_for_bit_as_the_scanpaths_they_were_rasterised_from():
    n = 0
    for p, (gt, gt_g), (pr, pr_g), shape, sigma, mode, _ in _golden_cases():
        G = max(gt_g) + 1
        given, _ = S().fixation_maps(pr, pr_g, (240, 320), shape, "count", num_groups=G)
        for kw in ({}, EXTRA):
            a = S().scanpath_saliency(gt, gt_g, pr, pr_g, (240, 320), sigma, output_shape=shape, mode=mode, **kw)
            for maps in (given, given.cpu().numpy()):                    # device or host
                b = S().scanpath_saliency(gt, gt_g, [], [], (240, 320), sigma, output_shape=shape, mode=mode, prediction="maps",
                                          pred_maps=maps, **kw)
                assert sorted(a) == sorted(b)
                for k in a:
                    if k != "pred_dropped":
                        assert torch.equal(_bits(a[k]), _bits(b[k])), (p, k, bool(kw))
                assert not b["pred_dropped"].any() and b["pred_dropped"].dtype == torch.int32
        n += 1
    assert n >= 6
    gt, gt_g = [np.array([[10.0, 10.0]])], [0]
    for bad in (float("nan"), float("inf"), -1.0):
        m = torch.ones(1, 240, 320, dtype=torch.float64, device=dev())
        m[0, 5, 5] = bad
        with pytest.raises(ValueError, match="finite, non-negative"):
            S().scanpath_saliency(gt, gt_g, [], [], (240, 320), 3.0, prediction="maps", pred_maps=m)


def test_scanpaths_and_centre_prior_are_unchanged():
    """prediction="scanpaths" and "centre_prior" on the golden end-to-end cases, with all four extras, against
    tests/golden/saliency_before_maps.npz: what the parent commit's scanpath_saliency (before the pred_maps branch existed) returned
    for the same calls on an MI355X, bit for bit"""
    before = load_npz(os.path.join(GOLDEN, "saliency_before_maps.npz"))
    n = 0
    for p, (gt, gt_g), (pr, pr_g), shape, sigma, mode, gold in _golden_cases():
        runs = {"scanpaths": S().scanpath_saliency(gt, gt_g, pr, pr_g, (240, 320), sigma, output_shape=shape, mode=mode, **EXTRA),
                "centre_prior": S().scanpath_saliency(gt, gt_g, [], [], (240, 320), sigma, output_shape=shape, mode=mode,
                                                      prediction="centre_prior", **EXTRA)}
        for name, res in runs.items():
            assert sorted(res) == sorted(k.split("/")[-1] for k in before if k.startswith(p + name + "/"))
            for k, v in res.items():
                same(v, before[p + name + "/" + k], (p, name, k))
        for k, r in (("AUC_Judd", gold[p + "auc"]), ("NSS", gold[p + "nss"]), ("KLdiv", gold[p + "kld"])):   # and the reference's values
            v = runs["scanpaths"][k].cpu().numpy()
            with np.errstate(all="ignore"):
                err = np.nanmax(np.abs(v - r) / (np.where(r != 0, np.abs(r), 1.0) if k == "KLdiv" else 1.0))
            assert np.array_equal(np.isnan(v), np.isnan(r)) and err <= 1e-9, (p, k, err)
        n += 1
    assert n >= 6


# ---- the keyed call, the table, the loop --------------------------------------------------------------------------------------------------
def _subjects(g, n):
    return [np.stack([g.uniform(0, 64, k), g.uniform(0, 48, k), g.uniform(0.1, 0.5, k)], 1) for k in g.integers(1, 7, n)]


def test_keyed_evaluation_equals_the_direct_composition(monkeypatch):
    from scanpaths_amd.utils import evaluation as E
    g = np.random.default_rng(51)
    N, T, shape, frame = 4, 5, (6, 8), (48, 64)
    A = 1 + shape[0] * shape[1]
    mk = lambda: g.dirichlet(np.ones(A), (N, T)).astype(np.float32)                         # noqa: E731
    host = {h + "all_actions_prob": mk() for h in ("", "good_", "poor_")}
    for h in ("", "good_", "poor_"):
        host[h + "log_normal_mu"] = g.uniform(-2.0, -1.0, (N, T)).astype(np.float32)
        host[h + "log_normal_sigma2"] = g.uniform(0.1, 0.6, (N, T)).astype(np.float32)
    host["all_actions_prob"][3, 1, 1:] = 0.0                                                # sample 3: a step without cell mass, bad as
    predict = {k: torch.from_numpy(v).to(dev()) for k, v in host.items()}                  # terminate is masked at t = 1
    keys = ["a", "b", "a", "c"]
    performances = [[True, False, True], [False], [True], [True, True]]
    fix_vectors = [_subjects(g, len(p)) for p in performances]
    kw = dict(sigma=2.0, min_length=2, max_steps=4, frame_size=frame, map_shape=shape)
    flat = [fv for s in fix_vectors for fv in s]
    # one head: one row per subject, every subject of a sample reads the sample's row
    rows, key_of = [0, 0, 0, 1, 2, 3, 3], [0, 0, 0, 1, 0, 2, 2]
    for weight, extra in (("count", ()), ("duration", ("CC", "SIM")), ("count", ALL)):
        more = dict(uniform_mix=0.01) if "IG" in extra else {}
        means, per_key = E.saliency_model_evaluation(predict, fix_vectors, keys, pred_weight=weight, extra_metrics=extra, **more, **kw)
        sw = S().expected_durations(host["log_normal_mu"], host["log_normal_sigma2"])[rows] if weight == "duration" else None
        direct = S().expected_fixation_maps(predict["all_actions_prob"][rows], key_of, 3, min_length=2, max_steps=4, frame_size=frame,
                                            map_shape=shape, step_weight=sw)
        assert direct["bad"].tolist() == [0, 0, 0, 0, 0, 1, 1]
        scores = S().scanpath_saliency(flat, key_of, [], [], frame, 2.0, num_groups=3, prediction="maps", pred_maps=direct["maps"],
                                       **(dict(extra_metrics=extra, image_groups=None, **more) if extra else {}))
        metrics = ("AUC_Judd", "NSS", "KLdiv") + tuple(extra)
        assert per_key["keys"] == ["a", "b", "c"] and set(per_key) == {"keys", "gt_dropped", "pred_dropped", "fixations"} | set(metrics)
        for m in metrics:
            same(per_key[m], scores[m].cpu().numpy(), (weight, m))
            ok = ~np.isnan(per_key[m])
            assert means[m + "_count"] == ok.sum() and means[m + "_sum"] == float(per_key[m][ok].sum()) and means[m + "_nan"] == (~ok).sum()
            assert means[m] == per_key[m][ok].mean() if ok.any() else np.isnan(means[m])
        assert not bool(direct["maps"][2].any()) and bool(direct["maps"][:2].any())           # key c: only bad rows, a zero map, scored
        assert not np.isnan(per_key["NSS"][:2]).any()                                            # as scanpath_saliency scores one
        f = direct["fixations"]
        same(per_key["fixations"], np.array([(f[0] + f[1] + f[2] + f[4]) / 4, f[3], np.nan]), "fixations per row")
        assert means["rows_count"] == 5 and means["rows_bad"] == 2 and means["fixations_sum"] == float(f[:5].sum())
    # the two AiR heads: the rows training assigns
    seen = {}
    real = S().expected_fixation_maps

    def spy(probs, row_groups, n_groups, **k):
        seen["probs"], seen["weight"] = probs.cpu().numpy(), k["step_weight"]
        return real(probs, row_groups, n_groups, **k)

    monkeypatch.setattr(S(), "expected_fixation_maps", spy)
    means2, per_key2 = E.saliency_model_evaluation(predict, fix_vectors, keys, performances, pred_weight="duration", **kw)
    both = {k: np.concatenate([host["good_" + k], host["poor_" + k]], 0) for k in ("all_actions_prob", "log_normal_mu", "log_normal_sigma2")}
    rows2 = [0, N + 0, 0, N + 1, 2, 3, 3]                                                    # built by hand from performances
    assert np.array_equal(seen["probs"], both["all_actions_prob"][rows2])
    m64, s64 = both["log_normal_mu"][rows2].astype(np.float64), both["log_normal_sigma2"][rows2].astype(np.float64)
    assert np.array_equal(seen["weight"], np.exp(m64 + s64 * s64 / 2.0))
    monkeypatch.undo()
    direct2 = S().expected_fixation_maps(torch.from_numpy(both["all_actions_prob"][rows2]).to(dev()), key_of, 3, min_length=2, max_steps=4,
                                         frame_size=frame, map_shape=shape, step_weight=seen["weight"])
    scores2 = S().scanpath_saliency(flat, key_of, [], [], frame, 2.0, num_groups=3, prediction="maps", pred_maps=direct2["maps"])
    for m in ("AUC_Judd", "NSS", "KLdiv"):
        same(per_key2[m], scores2[m].cpu().numpy(), ("two heads", m))
    assert means2["rows_count"] == 7 and means2["rows_bad"] == 0 and not np.isnan(per_key2["fixations"]).any()
    # per_key feeds the bootstrap as saliency_evaluation's does
    res = E.bootstrap_evaluation(per_key2, replicates=50, seed=3)
    assert list(res) == ["AUC_Judd", "NSS", "KLdiv", "fixations"] and res["NSS"]["n_valid"] == 50
    assert abs(res["NSS"]["estimate"] - means2["NSS"]) <= 1e-12 * abs(means2["NSS"])
    # the table over two batches: sum / count over all keys
    table = E.SaliencyModelTable()
    parts = []
    for lo in (0, 2):
        sl = {k: v[lo:lo + 2] for k, v in predict.items()}
        parts.append(E.saliency_model_evaluation(sl, fix_vectors[lo:lo + 2], keys[lo:lo + 2], **kw))
        table.add(parts[-1][0])
    out = table.result()
    values = np.concatenate([pk["NSS"] for _, pk in parts])
    assert out["NSS_count"] == (~np.isnan(values)).sum() >= 3 and out["NSS"] == out["NSS_sum"] / out["NSS_count"] and out["rows_bad"] == 2
    assert abs(out["NSS"] - np.nanmean(values)) <= 4 * 2.0 ** -53 * abs(np.nanmean(values))
    # refusals that need the predict
    with pytest.raises(ValueError, match="a union over samples, not an expectation"):
        E.saliency_model_evaluation(predict, fix_vectors, keys, pred_weight="binary", **kw)
    lacking = {k: v for k, v in predict.items() if "log_normal_sigma2" not in k}
    with pytest.raises(ValueError, match="predict lacks 'log_normal_sigma2'"):
        E.saliency_model_evaluation(lacking, fix_vectors, keys, pred_weight="duration", **kw)
    with pytest.raises(ValueError, match="predict lacks 'good_log_normal_sigma2'"):
        E.saliency_model_evaluation(lacking, fix_vectors, keys, performances, pred_weight="duration", **kw)
    E.saliency_model_evaluation(lacking, fix_vectors, keys, **kw)                           # "count" does not read them


def _equal(a, b, what):
    assert type(a) is type(b) or (np.isscalar(a) and np.isscalar(b)), (what, type(a), type(b))
    if isinstance(a, dict):
        assert set(a) == set(b), (what, set(a) ^ set(b))
        for k in a:
            _equal(a[k], b[k], (what, k))
    elif isinstance(a, list):                                            # the keys: strings
        assert a == b, (what, a, b)
    else:
        assert np.array_equal(a, b, equal_nan=True), (what, a, b)


def test_saliency_loop_on_a_tiny_multihead_model(monkeypatch):
    from scanpaths_amd import hip, inference
    from scanpaths_amd.models.baseline_attention_multihead import baseline
    from scanpaths_amd.procedural import fill_module
    from scanpaths_amd.synth import make_batch
    from scanpaths_amd.utils import evaluation as E
    T, B = 3, 2
    batches = [make_batch("COCO_Search18", B, 240, 320, T, seed=9 + k) for k in range(2)]
    model = baseline(convLSTM_length=T)
    fill_module(model, 9, family="tame")
    model = model.to(dev())
    g = np.random.default_rng(4)
    humans = [[[np.stack([g.uniform(0, 320, n), g.uniform(0, 240, n), g.uniform(0.1, 0.5, n)], 1) for n in g.integers(2, 8, 3)]
               for _ in range(B)] for _ in batches]
    loader = [{"images": b["images"], "attention_maps": b["attention_maps"], "tasks": b["tasks"], "fix_vectors": humans[k],
               "question_ids": [f"s{2 * k}", f"s{2 * k + 1}"]} for k, b in enumerate(batches)]
    S().expected_cell_pixels((30, 40), (240, 320))                       # the table is made once per process, with the sampler's kernel
    L, Mlib = hip.lib(), hip.model_lib()
    launches, launch = [], Mlib.sp_model_fixation_expectation
    monkeypatch.setattr(Mlib, "sp_model_fixation_expectation", lambda *a: launches.append(1) or launch(*a))
    for name in ("sp_sample_actions", "sp_generate_scanpath", "sp_beam_search"):
        monkeypatch.setattr(L, name, lambda *a: (_ for _ in ()).throw(AssertionError("the saliency loop does not sample")))
    kw = dict(sigma=8.0, min_length=1, max_steps=3, extra_metrics=("CC", "SIM"))
    means, per_batch = inference.run_saliency_loop(model, loader, **kw)
    assert len(launches) == 2 and len(per_batch) == 2 and per_batch[1]["keys"] == ["s2", "s3"] and not model.training
    table = E.SaliencyModelTable()
    for k, b in enumerate(batches):
        with torch.no_grad():
            predict = model(b["images"].to(dev()), b["attention_maps"].to(dev()), b["tasks"].to(dev()))
        assert tuple(predict["all_actions_prob"].shape) == (B, T, 1201)
        ev, keyed = E.saliency_model_evaluation(predict, humans[k], loader[k]["question_ids"], **kw)
        _equal(per_batch[k], keyed, "loop per key")
        table.add(ev)
    _equal(means, table.result(), "the loop returns the table of its batches")
    assert means["rows_count"] == 12 and means["rows_bad"] == 0 and 12 <= means["fixations_sum"] <= 36 and means["NSS_count"] == 4
    assert 0.0 <= means["AUC_Judd"] <= 1.0 and -1.0 <= means["CC"] <= 1.0 and 0.0 <= means["SIM"] <= 1.0
    with pytest.raises(ValueError, match="a batch is not the dataset"):
        inference.run_saliency_loop(model, loader, sigma=8.0, min_length=1, max_steps=3, extra_metrics=("IG",), uniform_mix=0.01)
    assert len(launches) == 4                                            # (the two direct calls above launched too; the refusal did not)
