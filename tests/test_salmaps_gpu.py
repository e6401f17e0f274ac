"""Attention-map losses and saliency / scanpath metrics on the device against the REAL reference (tests/golden/salmaps.npz, written by
tests/golden/make_golden_salmaps.py from AiR/models/loss.py and AiR/utils/evaltools/visual_attention_metrics.py).

Losses: value and input gradient within max(10 |ref32 - ref64|, 1e-4 |ref64|) of the fp64 reference (norm-wise for gradients), the
refusals (a target that requires grad, double backward, no question pair), bit-identical repeats.  Metrics: AUC-Judd and NSS within
1e-12, KLdiv within 1e-12 relative, the NaN pattern identical, the batched call bitwise equal to the per-pair wrappers; TDE / Euclidean
distances with False / None where the reference has them.  Model level: an AiR model trained with the supervised loss plus
KLD_question_aligment and CC on its step maps -- the backward's masked-step skip (row_sparsity) gives torch.equal parameter gradients
and moves each sample's horizon out to the latest step either loss reaches."""
import os

import numpy as np
import pytest
import torch

from helpers import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def gold():
    return load_npz(os.path.join(GOLDEN, "salmaps.npz"))


def _loss_names(g):
    return sorted(k[len("loss/"):-len("/val64")] for k in g if k.startswith("loss/") and k.endswith("/val64"))


def _fn(name):
    from scanpaths_amd.models import loss as L
    return {"smoothl1": L.DurationSmoothL1Loss, "rayleigh": L.MLPRayleighDistribution, "nss": L.NSS, "cc": L.CC, "kld": L.KLD,
            "klditems": L.KLD_items, "ccterms": L.CC_terms, "ccmatch": L.CC_MatchLoss, "kldvla": L.KLD_visual_linguistic_alignment,
            "kldqa": L.KLD_question_aligment}[name.split("_")[0]]


def _run(g, name, noncontig=False):
    diff = [int(i) for i in g[f"loss/{name}/diff"]]
    args = []
    k = 0
    while f"loss/{name}/in{k}" in g:
        t = torch.from_numpy(g[f"loss/{name}/in{k}"]).to(DEV)
        if noncontig and k == 0 and t.dim() >= 2:       # same values, transposed storage: the reference's .view would refuse it
            t = t.transpose(-1, -2).contiguous().transpose(-1, -2)
        args.append(t.requires_grad_(k in diff))
        k += 1
    out = _fn(name)(*args)
    grads = []
    if diff:
        w = torch.from_numpy(g[f"loss/{name}/w"]).float().to(DEV)
        s = (out * w).sum() if out.dim() else out
        grads = torch.autograd.grad(s, [args[i] for i in diff])
    return out, grads, diff


@pytest.mark.parametrize("noncontig", [False, True])
def test_losses_match_the_reference(gold, noncontig):
    names = _loss_names(gold)
    assert len(names) >= 20
    rows = []
    for name in names:
        out, grads, diff = _run(gold, name, noncontig)
        torch.cuda.synchronize()
        v64, v32 = gold[f"loss/{name}/val64"], gold[f"loss/{name}/val32"]
        got = out.detach().double().cpu().numpy()
        assert got.shape == v64.shape, (name, got.shape, v64.shape)
        if np.isinf(v64).any():
            assert np.array_equal(np.isinf(got), np.isinf(v64)), (name, got, v64)
        else:
            bar = max(10 * np.linalg.norm(v32 - v64), 1e-4 * np.linalg.norm(v64), 1e-7)
            err = np.linalg.norm(got - v64)
            rows.append((name, "value", err / bar))
            assert err <= bar, (name, got, v64, bar)
        for i, gr in zip(diff, grads):
            ref = gold[f"loss/{name}/grad64_{i}"].astype(np.float64)
            bar = max(10 * float(gold[f"loss/{name}/err32_{i}"]), 1e-4 * float(gold[f"loss/{name}/grad64norm_{i}"]))
            err = np.linalg.norm(gr.double().cpu().numpy() - ref)
            rows.append((name, f"grad{i}", err / bar))
            assert gr.shape == ref.shape and err <= bar, (name, i, err, bar)
    worst = max(rows, key=lambda r: r[2])
    print(f"{len(names)} losses; worst err/bar {worst[2]:.3f} ({worst[0]} {worst[1]})")


def test_losses_are_bit_identical_across_calls(gold):
    for name in _loss_names(gold):
        a, ga, _ = _run(gold, name)
        b, gb, _ = _run(gold, name)
        assert torch.equal(a, b), name
        assert all(torch.equal(x, y) for x, y in zip(ga, gb)), name


def test_cc_terms_without_a_pair_is_the_scalar_zero(gold):
    out, _, _ = _run(gold, "ccterms_none")
    assert out.dim() == 0 and float(out) == 0.0


def test_losses_refuse_target_gradients_double_backward_and_an_empty_pair_list():
    from scanpaths_amd.models import loss as L
    x = torch.rand(2, 6, 8, device=DEV, requires_grad=True)
    y = torch.rand(2, 6, 8, device=DEV, requires_grad=True)
    for fn in (L.NSS, L.CC, L.KLD, L.KLD_items):
        with pytest.raises(RuntimeError, match="salmap|fixation"):
            fn(x, y)
    m = torch.ones(2, 6, device=DEV, requires_grad=True)
    with pytest.raises(RuntimeError, match="mask"):
        L.DurationSmoothL1Loss(x[:, :, 0], x[:, :, 1].detach(), m)
    with pytest.raises(RuntimeError, match="gt"):
        L.MLPRayleighDistribution(x[:, :, 0] + 1, y[:, :, 0], m.detach())
    loss = L.KLD(x, y.detach())
    (gx,) = torch.autograd.grad(loss, x, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gx.sum(), x)
    z = torch.randn(2, 3, 6, 8, device=DEV, requires_grad=True)
    boxes = torch.ones(2, 6, 8, 4, device=DEV)
    with pytest.raises(RuntimeError, match="no \\(sample, question object\\) pair"):
        L.KLD_question_aligment(z, boxes, torch.zeros(2, 4, device=DEV), torch.ones(2, 3, device=DEV))
    with pytest.raises(RuntimeError, match="question_objects_pos"):
        L.KLD_question_aligment(z, boxes.requires_grad_(True), torch.ones(2, 4, device=DEV), torch.ones(2, 3, device=DEV))


# ---- metrics -------------------------------------------------------------------------------------------------------------------
def _maps(g):
    k = 0
    out = []
    while f"metric/{k}/sal" in g:
        out.append((g[f"metric/{k}/sal"], g[f"metric/{k}/fix"]))
        k += 1
    return out


def _close(got, ref, tol, rel=False):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (got, ref)
    ok = ~np.isnan(ref)
    err = np.abs(got[ok] - ref[ok])
    if rel:
        err = err / np.maximum(np.abs(ref[ok]), 1e-300)
    assert (err <= tol).all(), (got, ref, err)


def test_saliency_metrics_match_the_reference(gold):
    from scanpaths_amd.hip import lib
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    maps = _maps(gold)
    assert max(int((f > 0).sum()) for _, f in maps) > lib().sp_saliency_metrics_lds_fixations()      # the global-scratch path runs
    auc_j, auc, nss, kld = [], [], [], []
    for k, (s, f) in enumerate(maps):
        np.random.seed(k)
        auc_j.append(M.AUC_Judd(s, f, jitter=True))
        auc.append(M.AUC_Judd(s, f, jitter=False))
        nss.append(M.NSS(s, f))
        kld.append(M.KLdiv(s, f))
    _close(auc_j, gold["metric_auc_jitter"], 1e-12)
    _close(auc, gold["metric_auc"], 1e-12)
    _close(nss, gold["metric_nss"], 1e-12)
    _close(kld, gold["metric_kld"], 1e-12, rel=True)
    # the batched call, one launch per shape: bitwise what the wrappers return
    for shape in {s.shape for s, _ in maps}:
        idx = [k for k, (s, _) in enumerate(maps) if s.shape == shape]
        S = np.stack([maps[k][0] for k in idx])
        F = np.stack([maps[k][1] for k in idx])
        a, n, d = (t.cpu().numpy() for t in M.saliency_metrics_pairs(S, F))
        for j, k in enumerate(idx):
            for got, ref in ((a[j], auc[k]), (n[j], nss[k]), (d[j], kld[k])):
                assert (np.isnan(got) and np.isnan(ref)) or got == ref, (k, got, ref)
        J = []
        for k in idx:
            np.random.seed(k)
            J.append(np.random.random(shape) / 10 ** 7)
        aj = M.saliency_metrics_pairs(S, F, np.stack(J))[0].cpu().numpy()
        for j, k in enumerate(idx):
            if maps[k][1].any():
                assert aj[j] == auc_j[k], (k, aj[j], auc_j[k])


def test_auc_judd_draws_the_jitter_like_the_reference():
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    s = np.random.default_rng(1).random((12, 16))
    f = np.zeros((12, 16))
    np.random.seed(3)
    M.AUC_Judd(s, f)                          # no fixation: returns before drawing
    M.AUC_Judd(s, f + (np.arange(f.size).reshape(f.shape) % 7 == 0))
    after = np.random.random()
    np.random.seed(3)
    np.random.random(s.shape)
    assert after == np.random.random()


def _paths(g):
    fix, off = g["tde_fix"], g["tde_off"]
    return [fix[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def test_scanpath_distances_match_the_reference(gold):
    from scanpaths_amd.utils.evaltools import visual_attention_metrics as M
    paths = _paths(gold)
    img = np.zeros((240, 320, 3))
    calls = {"eucl": lambda a, b: M.euclidean_distance(a, b),
             "tde_k1": lambda a, b: M.time_delay_embedding_distance(a, b, k=1),
             "tde_k3": lambda a, b: M.time_delay_embedding_distance(a, b, k=3),
             "tde_k3_haus": lambda a, b: M.time_delay_embedding_distance(a, b, k=3, distance_mode='Hausdorff'),
             "tde_k5_haus": lambda a, b: M.time_delay_embedding_distance(a, b, k=5, distance_mode='Hausdorff'),
             "tde_k2_bad": lambda a, b: M.time_delay_embedding_distance(a, b, k=2, distance_mode='Median'),
             "stdd": lambda a, b: M.scaled_time_delay_embedding_distance(a.copy(), b.copy(), img)}
    n = len(paths)
    for key, fn in calls.items():
        ref, flag = gold[f"tde/{key}"], gold[f"tde/{key}_flag"]
        for i in range(n):
            for j in range(n):
                v = fn(paths[i], paths[j])
                if flag[i, j] == 1:
                    assert v is False, (key, i, j, v)
                elif flag[i, j] == 2:
                    assert v is None, (key, i, j, v)
                else:
                    assert isinstance(v, float) and abs(v - ref[i, j]) <= 1e-12 * max(1.0, abs(ref[i, j])), (key, i, j, v, ref[i, j])
    # batched: one launch for every pair, the same bits as the per-pair calls
    pairs = [(i, j) for i in range(n) for j in range(n)]
    tde, eucl = M.tde_pairs(paths, pairs, k=0, max_dim=320.0, want_euclidean=True)
    tde, eucl = tde.cpu().numpy(), eucl.cpu().numpy()
    for p, (i, j) in enumerate(pairs):
        r = gold["tde/stdd"][i, j]
        assert (np.isnan(tde[p]) and np.isnan(r)) or abs(tde[p] - r) <= 1e-12, (i, j)
        e = gold["tde/eucl"][i, j]
        assert (np.isnan(eucl[p]) and np.isnan(e)) or abs(eucl[p] - e) <= 1e-12 * max(1.0, abs(e)), (i, j)


# ---- model level ---------------------------------------------------------------------------------------------------------------
def _expected_kld_steps(z, boxes, qm, dm):
    """(sample, object) -> the step KLD_question_aligment's min picks, restated in torch float64 (AiR/models/loss.py:142-170)"""
    B, T, P = z.shape
    x = torch.softmax(z.double(), -1)
    xs = x / (x.sum(-1, keepdim=True) + 1e-7)
    steps = {}
    for b in range(B):
        for m in range(qm.shape[1]):
            if qm[b, m] == 0:
                break
            q = boxes[b, ..., m].reshape(1, P).double()
            q = q / (q.sum(-1, keepdim=True) + 1e-7)
            kl = (q * torch.log(q / (xs[b] + 1e-7) + 1e-7)).sum(-1)
            kl[dm[b] == 0] = float("inf")
            steps[(b, m)] = int(torch.argmin(kl))
    return steps


def test_attention_losses_on_the_step_maps_reach_the_backward_skip(monkeypatch):
    from scanpaths_amd import functional as F
    from scanpaths_amd.models.loss import CC, KLD_question_aligment, supervised_loss
    from helpers import assert_same_grads as _assert_same_grads, build_model as _build, call_model as _call, param_grads as _grads, \
        sparsity_case as _sparsity_case
    if F.SPLIT_SCHEME != "f16x2" or not F.USE_BF16X3 or F.THROUGHPUT_MODE:      # the backend test_model_gpu's sparsity tests need
        pytest.skip("2xfp16 back-end not active")
    T, Hm, Wm, M = 8, 40, 64, 3
    meta, b = _sparsity_case("AiR", T=T)
    monkeypatch.setattr(F, "COST_M_SCALE", 32.0 / 5)
    B = b["action_masks"].shape[0]
    g = torch.Generator().manual_seed(11)
    boxes = torch.zeros(B, Hm, Wm, M)
    for i in range(B):
        for m in range(M):
            y0, x0 = int(torch.randint(0, Hm - 8, (1,), generator=g)), int(torch.randint(0, Wm - 8, (1,), generator=g))
            boxes[i, y0:y0 + 8, x0:x0 + 12, m] = 1.0
    boxes = boxes.to(DEV)
    qm = torch.tensor([[1, 1, 0], [1, 0, 0], [0, 0, 0], [1, 1, 1], [1, 0, 1]], dtype=torch.float32, device=DEV)
    dm = torch.ones(B, T, device=DEV)
    dm[:, 6:] = 0                                                  # the last two steps never take part in the alignment
    salmap = torch.rand(B, Hm, Wm, generator=g).to(DEV)
    cc_step = 1
    res = {}
    for sparse in (False, True):
        monkeypatch.setattr(F, "ROW_SPARSITY", sparse)
        model = _build(meta, Hm, Wm).train()
        pred = _call(model, meta, b)
        z = pred["all_actions_prob"]
        assert z.shape == (B, T, 1 + Hm * Wm), z.shape
        maps = z[..., 1:].reshape(B, T, Hm, Wm)
        loss, _, _ = supervised_loss(pred, b["scanpaths"], b["durations"], b["action_masks"], b["duration_masks"], 1.0)
        kqa = KLD_question_aligment(maps, boxes, qm, dm)
        cc = CC(maps[:, cc_step], salmap)
        total = loss + 1e-2 * kqa - 1e-2 * cc
        total.backward()
        torch.cuda.synchronize()
        rows = model.last_decode_rows
        if sparse:
            steps = _expected_kld_steps(z[..., 1:].detach(), boxes, qm, dm)
            sup_last = [0, 3, T - 1, 1, -1]                        # _sparsity_case's scanpath lengths (1, 4, 8, 2, 0)
            want = [max([sup_last[i], cc_step] + [t for (bb, _), t in steps.items() if bb == i]) for i in range(B)]
            assert rows.rc.last.tolist() == want, (rows.rc.last.tolist(), want, steps)
        else:
            assert rows.rc is None
        res[sparse] = (float(total.detach()), _grads(model))
    assert res[True][0] == res[False][0]
    _assert_same_grads(res[True][1], res[False][1])
